"""The phrase position check at its position edges, through each of the five kernels that write it out (-m gpu):

  dense     bm25_phrase_kernel<NT,KPL,PT>    dense phrases of <= 6 unique terms, k <= 128            search_lexical_batch
  gallop    bm25_gallop phrase instances     7 .. 12 unique terms, or k > 128, either tier           search_lexical_batch (generic_batches moves)
  sparse    bm25_sparse_phrase_kernel        phrases naming a sparse-tier term, staged               the device-pointer entry, ops-mask bit 28
  small     sm_phrase_wave                   the same, <= 4 unique terms, k <= 32, one launch        search_lexical_batch (one_launch_batches moves)
  refine    phrase_refine_kernel<PT>         match sets: facet counts, sorted pages, query_facets    facet_count / sorted_batch / search_lexical_facets

over the worlds of tests/phrase_edge_world.py: one indexed field (u16 positions) and three (field-tagged u32 positions), each untiered
and tiered.  The expectation is that module's definition and oracle/naive.py's exact scores -- never the device, never another device
path (tests/test_phrase_edge_world_cpu.py shows the worlds are what they claim).  Every route answers the world's phrase table with
tombstones off and on.  Per query: totals == the definition's count; returned count == min(k, matches); every returned doc a match (a
rich_miss / wrap / same / gap doc never); at k >= matches the returned set == the definition's; scores within 1e-4 relative of the exact
ones; at smaller k the ids above the k-th score's tie band (2e-4 |score_k|) are the definition's; Topk and
TopkCount agree bit for bit.  A failure names the route, the phrase and the docs that differ by their case names."""
import numpy as np
import pytest

import phrase_edge_world as PW
from test_gpu_small_batch import _dev_search, _same_answers

pytestmark = pytest.mark.gpu
REL = 1e-4    # test_gpu_score_edges.REL
BAND = 2e-4   # the suite's tie band around the k-th score
FORMS = [(1, "untiered"), (1, "tiered"), (2, "untiered"), (2, "tiered")]
TIERED = [f for f in FORMS if f[1] == "tiered"]
IDS = lambda forms: ["%s_%s" % ("u16" if w == 1 else "u32", f) for w, f in forms]
BOUNDS = [0, 2048, 4096, 6144, 8192]  # of the doc-id facet


@pytest.fixture(scope="module")
def S():
    import seekstorm_amd
    return seekstorm_amd


class Form:
    """one world uploaded in one form: the shard, and the term ids its names got"""

    def __init__(self, S, W, tiered):
        self.W, self.tiered, self.S = W, tiered, S
        self.sh = sh = S.Shard(0)
        dense = W.dense if tiered else W.untiered
        a = W.csr(dense)
        if W.n_fields == 1:
            sh.upload_lexical(W.n_docs, W.doclen, a[0], a[1], a[2], a[3])
        else:
            sh.upload_lexical_fields(W.n_docs, W.doclen, W.boost, a[0], a[1], a[2], a[3], a[4])
            assert sh.fields_info()[1:] == (True, True)  # merged lists, positions
        terms = list(dense)
        if tiered:
            b = W.csr(W.sparse)
            first = sh.append_sparse(b[0], b[1], b[2], positions=b[3]) if W.n_fields == 1 else \
                sh.append_sparse_fields(b[0], b[1], b[2], b[3], positions=b[4])
            assert first == len(dense)
            terms += W.sparse
        self.tid = {t: i for i, t in enumerate(terms)}
        sh.upload_facets(np.arange(W.n_docs, dtype="<u2").view(np.uint8).reshape(W.n_docs, 2))  # a 2-byte record: the doc id
        self.what = "%s, %s" % (W.name, "tiered" if tiered else "untiered")

    def names_sparse(self, ph):
        return self.tiered and bool(set(ph.uniq) & self.W.sparse_terms)

    def all_dense(self, ph):
        return not self.tiered or not (set(ph.uniq) | set(ph.nots)) & self.W.sparse_terms

    def queries(self, phrases):
        qs = [self.sh.make_queries([[self.tid[w] for w in ph.words]], self.S.QueryType.Phrase, [[self.tid[t] for t in ph.nots]],
                                   field_filter=ph.filt or None) for ph in phrases]
        return np.concatenate(qs)


@pytest.fixture(scope="module")
def forms(S):
    made = {}

    def get(which, form):
        if (which, form) not in made:
            made[(which, form)] = Form(S, PW.world(which), form == "tiered")
        return made[(which, form)]
    yield get
    for f in made.values():
        f.sh.close()


def check(F, route, phrases, k, rt, res, dead):
    """the answers of one call against the definition"""
    S, W = F.S, F.W
    doc, score, cnt, tot = res
    for i, ph in enumerate(phrases):
        where = "%s | %s | %s | k = %d, %s, %s" % (route, F.what, ph, k, rt.name, "tombstones" if dead else "live")
        ed, es = W.expected(ph, dead)
        n = len(ed)
        total = "%s: total %d, the definition counts %d" % (where, int(tot[i]), n)
        if rt == S.ResultType.Count:
            assert int(tot[i]) == n, total
            continue
        c = int(cnt[i])
        got = doc[i][:c].astype(np.int64)
        wrong = sorted(set(got.tolist()) - set(ed.tolist()))
        assert not wrong, "%s: returned docs that hold no match: %s" % (where, W.names(wrong))
        missing = W.names(set(ed[:k].tolist()) - set(got.tolist()))
        assert c == min(k, n), "%s: %d results, want min(k, %d matches); not returned: %s" % (where, c, n, missing)
        assert len(set(got.tolist())) == c, "%s: a doc twice" % where
        if k >= n:
            assert set(got.tolist()) == set(ed.tolist()), "%s: not returned: %s" % (where, missing)
        if c:
            own = dict(zip(ed.tolist(), es.tolist()))
            gs = score[i][:c].astype(np.float64)
            exact = np.array([own[int(d)] for d in got])
            bad = np.abs(gs - exact) > REL * np.abs(exact)
            assert not bad.any(), "%s: %s scored %.7g, exact %.7g" % (where, W.names(got[bad][:1]), gs[bad][0], exact[bad][0])
            assert np.all(gs[1:] <= gs[:-1]), "%s: scores out of order" % where
            kth = float(es[c - 1])
            band = BAND * abs(kth)
            must = {int(d) for d, s in zip(ed, es) if s > kth + band}
            assert must <= set(got.tolist()), "%s: above the tie band and not returned: %s" % (where, W.names(must - set(got.tolist())))
            low = [int(d) for d, s in zip(got, exact) if s < kth - band]
            assert not low, "%s: returned from below the tie band: %s" % (where, W.names(low))
        if rt == S.ResultType.TopkCount:
            assert int(tot[i]) == n, total


def same_topk(F, route, phrases, k, a, b):
    """Topk and TopkCount agree on docs and scores"""
    for i, ph in enumerate(phrases):
        c = int(a[2][i])
        assert c == int(b[2][i]) and np.array_equal(a[0][i][:c], b[0][i][:c]) and np.array_equal(a[1][i][:c].view(np.uint32), b[1][i][:c].view(np.uint32)), \
            "%s | %s | %s | k = %d: Topk and TopkCount differ: %s" % (route, F.what, ph, k, F.W.names(np.setxor1d(a[0][i][:c], b[0][i][:int(b[2][i])])))


def run_host(F, route, phrases, k, dead, rts=None):
    """search_lexical_batch of the phrases as ONE call, checked for every result type"""
    S = F.S
    q = F.queries(phrases)
    res = {}
    for rt in rts or (S.ResultType.TopkCount, S.ResultType.Topk, S.ResultType.Count):
        res[rt] = F.sh.search_lexical_batch(q, k, rt, reference_shortcuts=False)
        check(F, route, phrases, k, rt, res[rt], dead)
    same_topk(F, route, phrases, k, res[S.ResultType.Topk], res[S.ResultType.TopkCount])
    return len(res)


def nt_class(ph):
    """the instantiation of bm25_phrase_kernel a batch of such phrases takes: NT = 2, 3, 4, 6"""
    n = len(ph.uniq)
    return 2 if n <= 2 else n if n <= 4 else 6


# ------------------------------------------------------------------------------------------------ bm25_phrase_kernel
@pytest.mark.parametrize("dead", [False, True], ids=["live", "tombstones"])
@pytest.mark.parametrize("which,form", FORMS, ids=IDS(FORMS))
def test_dense_phrase_kernel(S, forms, which, form, dead):
    """dense phrases of <= 6 unique terms, k = 1 / 10 / 100: every phrase alone (one query per call), then as batches of 2, 3, 4 and
    5 .. 6 unique terms in calls of their own (NT = 2, 3, 4, 6).  Neither the one-launch path nor the generic kernel answers them."""
    F = forms(which, form)
    phrases = [ph for ph in F.W.table if len(ph.uniq) <= 6 and F.all_dense(ph)]
    assert phrases
    if not F.tiered:
        assert {nt_class(ph) for ph in phrases} == ({2, 3, 4, 6} if which == 1 else {2, 3})
    F.sh.set_deleted(F.W.gone if dead else [])
    try:
        before = (F.sh.one_launch_batches(), F.sh.generic_batches())
        for k in (100, 10, 1):  # (the whole set first: a failure there names every doc that differs)
            for ph in phrases:
                run_host(F, "dense, alone", [ph], k, dead)
            for nt in sorted({nt_class(ph) for ph in phrases}):
                run_host(F, "dense, batch NT = %d" % nt, [ph for ph in phrases if nt_class(ph) == nt], k, dead)
        assert (F.sh.one_launch_batches(), F.sh.generic_batches()) == before, "a dense phrase of <= 6 terms left bm25_phrase_kernel"
    finally:
        F.sh.set_deleted([])


# ------------------------------------------------------------------------------------------------ bm25_gallop
@pytest.mark.parametrize("dead", [False, True], ids=["live", "tombstones"])
@pytest.mark.parametrize("which,form", FORMS, ids=IDS(FORMS))
def test_gallop_phrase_kernel(S, forms, which, form, dead):
    """phrases of 7 and of 12 unique terms at k = 1 / 10 / 100, and the two-word phrases of either tier at k = 129: generic_batches
    moves with every call"""
    F = forms(which, form)
    long = [ph for ph in F.W.table if len(ph.uniq) > 6]
    short = [ph for ph in F.W.table if len(ph.words) == 2]
    assert {len(ph.uniq) for ph in long} == ({7, 12} if which == 1 else {7}) and len(short) >= 5
    if F.tiered:
        assert all(F.all_dense(ph) for ph in long) and any(F.names_sparse(ph) for ph in short)
    F.sh.set_deleted(F.W.gone if dead else [])
    try:
        # (a Count request carries no k: a two-word phrase's count is its own kernel's, not the generic one's)
        for phrases, ks, rts in ((long, (100, 10, 1), None), (short, (129,), (S.ResultType.TopkCount, S.ResultType.Topk))):
            for k in ks:
                for group in [phrases] + [[ph] for ph in phrases[:2]]:
                    before = F.sh.generic_batches()
                    one = F.sh.one_launch_batches()
                    calls = run_host(F, "gallop", group, k, dead, rts)
                    assert F.sh.generic_batches() == before + calls and F.sh.one_launch_batches() == one, ("not the generic kernel", F.what, group, k)
    finally:
        F.sh.set_deleted([])


@pytest.mark.parametrize("which", [1, 2], ids=["u16", "u32"])
def test_seven_terms_with_a_sparse_one_stay_with_the_caller(S, forms, which):
    """the match-set entries keep the staged sparse kernel's limit (seekstorm_hip.h, ss_bm25_facet_count): a phrase of more than 6 unique
    terms that names a sparse term is SS_ENOTSUP there"""
    from seekstorm_amd import _native as N
    F = forms(which, "tiered")
    ph = PW.Phrase(tuple(PW.T7[:6]) + ("A",))
    assert len(ph.uniq) == 7 and F.names_sparse(ph)
    with pytest.raises(N.SeekStormHipError) as e:
        F.sh.facet_count(F.queries([ph]), 0, "u16", range_lower_bounds=BOUNDS)
    assert e.value.code == N.SS_ENOTSUP


# ------------------------------------------------------------------------------------------------ bm25_sparse_phrase_kernel, sm_phrase_wave
def sparse_named(F):
    return [ph for ph in F.W.table if F.names_sparse(ph) and len(ph.uniq) <= 6]


@pytest.mark.parametrize("dead", [False, True], ids=["live", "tombstones"])
@pytest.mark.parametrize("which,form", TIERED, ids=IDS(TIERED))
def test_staged_sparse_phrase_kernel(S, forms, which, form, dead):
    """phrases naming a sparse term -- sparse-sparse, sparse-dense, dense-sparse, repeated, NOT terms of either tier, field filters --
    through the device-pointer entry, which is the staged tiered pipeline by construction"""
    F = forms(which, form)
    phrases = sparse_named(F)
    shapes = {tuple(w in F.W.sparse_terms for w in ph.words) for ph in phrases}
    assert {(True, True), (True, False), (False, True)} <= shapes
    F.sh.set_deleted(F.W.gone if dead else [])
    try:
        before = (F.sh.one_launch_batches(), F.sh.generic_batches())
        for k in (100, 10, 1):  # (the whole set first: a failure there names every doc that differs)
            for group in [phrases] + [[ph] for ph in phrases[:3]]:
                q = F.queries(group)
                res = {}
                for rt in (S.ResultType.TopkCount, S.ResultType.Topk, S.ResultType.Count):
                    res[rt] = _dev_search(S, F.sh, q, k, rt, (1 << 28) | 16)
                    check(F, "staged sparse", group, k, rt, res[rt], dead)
                same_topk(F, "staged sparse", group, k, res[S.ResultType.Topk], res[S.ResultType.TopkCount])
        assert (F.sh.one_launch_batches(), F.sh.generic_batches()) == before
    finally:
        F.sh.set_deleted([])


@pytest.mark.parametrize("dead", [False, True], ids=["live", "tombstones"])
@pytest.mark.parametrize("which,form", TIERED, ids=IDS(TIERED))
def test_one_launch_phrase_wave(S, forms, which, form, dead):
    """the same phrases of <= 4 unique terms at k <= 32 through search_lexical_batch: one launch (role 3), bit-equal to the staged
    kernel.  Under a field filter (three fields) a phrase does not take the one launch: the staged kernel answers it."""
    F = forms(which, form)
    phrases = [ph for ph in sparse_named(F) if len(ph.uniq) <= 4 and not ph.filt]
    filtered = [ph for ph in sparse_named(F) if ph.filt]
    assert len(phrases) >= 5 and bool(filtered) == (which == 2)
    F.sh.set_deleted(F.W.gone if dead else [])
    try:
        for k in (32, 10, 1):
            for group in [phrases] + [[ph] for ph in phrases[:3]]:
                q = F.queries(group)
                for rt in (S.ResultType.TopkCount, S.ResultType.Topk):
                    before = F.sh.one_launch_batches()
                    got = F.sh.search_lexical_batch(q, k, rt, reference_shortcuts=False)
                    assert F.sh.one_launch_batches() == before + 1, ("not one launch", F.what, group, k, rt)
                    check(F, "one launch", group, k, rt, got, dead)
                    _same_answers(got, _dev_search(S, F.sh, q, k, rt, (1 << 28) | 16), rt, S, ("one launch vs staged", F.what, k, rt))
            if filtered:
                before = F.sh.one_launch_batches()
                run_host(F, "staged sparse (field filter)", filtered, k, dead)
                assert F.sh.one_launch_batches() == before, "a phrase under a field filter took the one launch"
    finally:
        F.sh.set_deleted([])


# ------------------------------------------------------------------------------------------------ phrase_refine_kernel
@pytest.mark.parametrize("dead", [False, True], ids=["live", "tombstones"])
@pytest.mark.parametrize("which,form", FORMS, ids=IDS(FORMS))
def test_refined_match_sets(S, forms, which, form, dead):
    """the match sets behind facet counts, sorted pages and query_facets, over a 2-byte facet record that holds the doc id: the
    histogram of every phrase == the definition's (it sums to the match count); the page sorted ascending on that column at k = 128 lists
    exactly the match set in doc order; search_lexical_facets returns search_lexical_batch's hits bit for bit, and the same histograms"""
    F = forms(which, form)
    W, sh = F.W, F.sh
    phrases = list(W.table)
    sh.set_deleted(W.gone if dead else [])
    try:
        want = [W.matches(ph, dead) for ph in phrases]
        hist = [np.bincount(np.searchsorted(BOUNDS, m, side="right") - 1, minlength=len(BOUNDS)).astype(np.uint64) for m in want]
        for ph, m, h in zip(phrases, want, hist):
            counts, other, tot = sh.facet_count(F.queries([ph]), 0, "u16", range_lower_bounds=BOUNDS)
            where = "refine, facet_count | %s | %s | %s" % (F.what, ph, "tombstones" if dead else "live")
            assert tot == len(m) == int(counts.sum()) + other and other == 0, "%s: %d docs counted, total %d, the definition counts %d" % (where, int(counts.sum()), tot, len(m))
            assert np.array_equal(counts, h), "%s: per sub-range %s, want %s" % (where, counts.tolist(), h.tolist())
        q = F.queries(phrases)
        doc, score, cnt, tot = sh.search_lexical_sorted_batch(q, [(0, "u16", False)], 128)
        for i, (ph, m) in enumerate(zip(phrases, want)):
            where = "refine, sorted page | %s | %s | %s" % (F.what, ph, "tombstones" if dead else "live")
            got = doc[i][:int(cnt[i])].astype(np.int64)
            assert int(tot[i]) == len(m) and np.array_equal(got, m), "%s: total %d (want %d); differ on %s" % (where, int(tot[i]), len(m), W.names(np.setxor1d(got, m)))
            own = W.scores(ph.uniq)
            exact = np.array([own[int(d)] for d in got])
            assert np.all(np.abs(score[i][:len(got)] - exact) <= REL * np.abs(exact)), where
        qfs = [{"field": "id", "offset": 0, "type": "u16", "ranges": [("r%d" % i, b) for i, b in enumerate(BOUNDS)], "range_type": "within"}]
        for rt in (S.ResultType.TopkCount, S.ResultType.Topk):
            d1, s1, c1, t1, per = sh.search_lexical_facets(q, 10, qfs, rt, reference_shortcuts=False)
            d2, s2, c2, t2 = sh.search_lexical_batch(q, 10, rt, reference_shortcuts=False)
            where = "refine, search_lexical_facets | %s | %s | %s" % (F.what, rt.name, "tombstones" if dead else "live")
            assert np.array_equal(d1, d2) and np.array_equal(s1.view(np.uint32), s2.view(np.uint32)) and np.array_equal(c1, c2) and np.array_equal(t1, t2), where
            check(F, "refine, search_lexical_facets", phrases, 10, rt, (d1, s1, c1, t1), dead)
            for i, ph in enumerate(phrases):
                assert np.array_equal(per[0][i][:len(BOUNDS)], hist[i]) and int(per[0][i][len(BOUNDS)]) == 0, "%s | %s: %s, want %s" % (where, ph, per[0][i].tolist(), hist[i].tolist())
    finally:
        sh.set_deleted([])
