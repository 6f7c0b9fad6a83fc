"""BM25 scores at the edges of the posting's weight code (ss_common.h bm_wcode: [2^-14, 4), 15 mantissa bits).

Every answer of every kernel family is compared with naive.bm25_exact -- the crate's f32 factors summed in float64 -- not with
another device strategy (they share the code and would agree on a clamped weight):
  counts exact, every score within 1e-4 relative of the exact one, docs above the tie band the reference's, bit-equal reference
  groups in doc-id order.
Corpora: a giant doc in the code's lowest binade (the 16-bit scan's denormal fold) and one below it (no code: the upload must
refuse it with SS_ENOTSUP, never clamp it), a mostly empty corpus, idf / tf extremes, exact ties, three indexed fields, an
incremental image whose commits push earlier postings out of range, and phrases naming unique terms past the phrase kernels' 12 slots.
"""
import numpy as np
import pytest

from oracle import naive

pytestmark = pytest.mark.gpu
REL = 1e-4
KS = (1, 10, 33, 100, 129, 1024, 1500)


@pytest.fixture(scope="module")
def S():
    import seekstorm_amd
    return seekstorm_amd


@pytest.fixture(scope="module")
def N():
    from seekstorm_amd import _native
    return _native


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


def _b4(words):
    return np.array([naive.int_to_byte4(int(x)) for x in np.atleast_1d(words)], np.uint8)


def _len_for_ratio(doclen, at, lo, hi):
    """a SmallFloat length for doc `at` whose tf = 1 weight, with doclen[at] set to it, lies in [lo, hi)"""
    for b in range(255, 0, -1):
        dl = doclen.copy()
        dl[at] = b
        comp = naive.component_cache(naive.avgdl(dl))
        w = np.float32(2.2) / (np.float32(1.0) + comp[b])
        if lo <= w < hi:
            return b
    raise AssertionError("no length byte gives that weight")


def _weight_tf1(doclen, at):
    comp = naive.component_cache(naive.avgdl(doclen))
    return float(np.float32(2.2) / (np.float32(1.0) + comp[doclen[at]]))


class Corpus:
    def __init__(self, n_docs, doclen, lists):
        self.n_docs, self.doclen = n_docs, np.asarray(doclen, np.uint8)
        self.lists = [(np.asarray(d, np.uint32), np.asarray(t, np.uint16)) for d, t in lists]
        self.offs = np.zeros(len(lists) + 1, np.uint64)
        self.offs[1:] = np.cumsum([len(d) for d, _ in self.lists])
        self.docs = np.concatenate([d for d, _ in self.lists])
        self.tfs = np.concatenate([t for _, t in self.lists])
        self._ref = {}

    def ref(self, terms, op_and, nots=(), deleted=()):
        key = (tuple(terms), op_and, tuple(nots), tuple(int(x) for x in deleted))
        if key not in self._ref:
            ids, sc = naive.bm25_exact(self.n_docs, self.doclen, [self.lists[t] for t in terms], op_and,
                                       not_docs=[self.lists[t][0] for t in nots], deleted=np.asarray(deleted, np.int64))
            order = np.lexsort((ids, -sc))
            self._ref[key] = (ids, sc, ids[order].astype(np.int64), sc[order])
        return self._ref[key]


def _gen(n_docs, doclen, specs, seed):
    """specs: (df or explicit doc array, tf rule) -> Corpus"""
    rng = np.random.default_rng(seed)
    lists = []
    for docs, tf in specs:
        if not isinstance(docs, np.ndarray):
            docs = np.sort(rng.choice(n_docs, max(1, int(docs * n_docs)), replace=False))
        docs = np.unique(docs).astype(np.uint32)
        if callable(tf):
            tfs = tf(rng, docs)
        else:
            tfs = np.full(len(docs), tf, np.uint16)
        lists.append((docs, np.asarray(tfs, np.uint16)))
    return Corpus(n_docs, doclen, lists)


def _geo(rng, docs):
    return rng.geometric(0.5, len(docs)).clip(1, 300).astype(np.uint16)


def _check(c, where, terms, op_and, nots, deleted, k, rt, d, s, cnt, tot, S, exact_ties=False):
    ids, sc, rd, rs = c.ref(terms, op_and, nots, deleted)
    total = len(ids)
    if rt != S.ResultType.Topk:
        assert int(tot) == total, f"{where}: result_count_total {int(tot)} != {total}"
    if rt == S.ResultType.Count:
        return
    n = min(k, total)
    assert int(cnt) == n, f"{where}: {int(cnt)} results, want {n}"
    if n == 0:
        return
    dd = d[:n].astype(np.int64)
    ds = s[:n].astype(np.float64)
    assert len(np.unique(dd)) == n, f"{where}: a doc twice"
    pos = np.searchsorted(ids, dd)
    assert np.all(pos < len(ids)) and np.all(ids[np.minimum(pos, len(ids) - 1)] == dd), f"{where}: a doc that does not match"
    own = sc[pos]
    bad = np.abs(ds - own) > REL * np.abs(own)
    assert not bad.any(), f"{where}: doc {dd[bad][0]} scored {ds[bad][0]:.7g}, exact {own[bad][0]:.7g} ({(ds[bad][0] / own[bad][0] - 1) * 100:+.1f} %)"
    assert np.all(np.abs(ds - rs[:n]) <= REL * np.abs(rs[:n])), f"{where}: the k-th scores differ from the reference's"
    kth = rs[n - 1]
    band = abs(kth) * REL
    assert set(dd[own > kth + band].tolist()) == set(rd[:n][rs[:n] > kth + band].tolist()), f"{where}: docs above the tie band differ"
    assert np.all(ds[1:] <= ds[:-1]), f"{where}: scores out of order"
    # bit-equal groups (the reference's sums, and the device's own: terms of equal idf whose tfs trade places sum to one float64 value
    # but to f32 chains an ulp apart) in doc-id order
    eq = (own[1:] == own[:-1]) & (ds[1:] == ds[:-1])
    assert np.all(dd[1:][eq] > dd[:-1][eq]), f"{where}: bit-equal scores out of doc-id order"
    if exact_ties:
        assert np.array_equal(dd, rd[:n]), f"{where}: equal scores must come back lowest doc ids first"


def _queries(S, sh, terms_list, op, nots_list=None):
    qt = S.QueryType.Intersection if op else S.QueryType.Union
    return sh.make_queries(terms_list, qt, nots_list)


def _run_all(S, N, sh, c, qsets, deleted=(), strategies=None, ks=KS, exact_ties=False):
    """qsets: list of (terms, op_and, nots).  Every strategy x batch form x k x result type the query takes."""
    strategies = strategies or (N.BM25_AUTO, N.BM25_EXHAUSTIVE, N.BM25_EXHAUSTIVE_F32, N.BM25_PRUNED)
    for strat in strategies:
        sh.set_strategy(strat)
        try:
            for op_and in (False, True):
                qs = [q for q in qsets if q[1] == op_and and (strat != N.BM25_PRUNED or len(q[0]) <= 4)]
                if not qs:
                    continue
                q = _queries(S, sh, [x[0] for x in qs], op_and, [list(x[2]) for x in qs])
                # batch forms: all at once (> 64: the staged pipeline), 64 at a time and one at a time (the one-launch kernel)
                forms = [("all", [np.arange(len(qs))])]
                if len(qs) > 64:
                    forms.append(("64", [np.arange(i, min(i + 64, len(qs))) for i in range(0, len(qs), 64)]))
                forms.append(("1", [np.array([i]) for i in range(0, len(qs), max(1, len(qs) // 6))]))
                for form, chunks in forms:
                    for k in ks:
                        rts = (S.ResultType.Topk, S.ResultType.TopkCount, S.ResultType.Count) if form == "all" else (S.ResultType.TopkCount,)
                        for rt in rts:
                            if rt == S.ResultType.Count and k != 10:
                                continue
                            for ch in chunks:
                                try:
                                    d, s, cnt, tot = sh.search_lexical_batch(q[ch], k, rt, reference_shortcuts=False)
                                except N.SeekStormHipError as e:  # (the explicit pruned strategy refuses what pruning cannot serve)
                                    assert strat == N.BM25_PRUNED and e.code == N.SS_ENOTSUP, e
                                    continue
                                for j, i in enumerate(ch):
                                    terms, _, nots = qs[i]
                                    where = f"strategy {strat} batch {form} k={k} rt={int(rt)} {'AND' if op_and else 'OR'} {terms} NOT {list(nots)}"
                                    _check(c, where, terms, op_and, nots, deleted, k, rt, d[j], s[j], cnt[j], tot[j], S, exact_ties)
        finally:
            sh.set_strategy(N.BM25_AUTO)


def _std_queries(rng, n_terms, giant_terms):
    """1..4-term unions and 2 / 3-term intersections, 7 / 12 / 32-term unions, NOT terms; every query names a giant-doc term"""
    out = []
    for t in range(n_terms):
        out.append(([t], False, ()))
    for _ in range(40):
        m = int(rng.integers(2, 5))
        ts = [int(giant_terms[rng.integers(len(giant_terms))])] + [int(x) for x in rng.choice(n_terms, m + 2, replace=False)]
        ts = list(dict.fromkeys(ts))[:m]
        out.append((ts, False, ()))
        out.append((ts[:2 + (m > 2)], True, ()))
    for m in (7, 12, 32):
        if m <= n_terms:
            out.append(([int(x) for x in rng.permutation(n_terms)[:m]], False, ()))
    for _ in range(8):
        ts = [int(x) for x in rng.choice(n_terms, 4, replace=False)]
        out.append((ts[:3], False, (ts[3],)))
        out.append((ts[:2], True, (ts[3],)))
    return out


def _try_upload(S, N, sh, c):
    try:
        sh.upload_lexical(c.n_docs, c.doclen, c.offs, c.docs, c.tfs)
        return True
    except N.SeekStormHipError as e:
        assert e.code == N.SS_ENOTSUP, e
        return False


def _giant_corpus(m, lo, hi, seed):
    """short docs (10..30 words), giant docs at 4095 and n_docs - 1 (n_docs = 4096 m + 1), a few docs of length byte 0; the giant
    doc 4095's tf = 1 weight in [lo, hi), the other twice as long; terms with df 1, 2, N - 1, N, tf 9 / 10 on a flagged list, tf 65535"""
    rng = np.random.default_rng(seed)
    n = 4096 * m + 1
    dl = _b4(rng.integers(10, 31, n))
    dl[rng.choice(n, 50, replace=False)] = 0
    g = np.array([4095, n - 1])
    dl[n - 1] = _b4(2_000_000)[0]
    dl[4095] = _len_for_ratio(dl, 4095, lo, hi)
    for _ in range(3):  # (the giant docs' own lengths move avgdl: settle both)
        dl[n - 1] = dl[4095]
        dl[4095] = _len_for_ratio(dl, 4095, lo, hi)
    dl[n - 1] = dl[4095]
    every = np.arange(n)
    flag_tf = lambda r, d: np.where(r.random(len(d)) < 0.5, 9, 10).astype(np.uint16)
    specs = [
        (np.array([4095]), 1),                                   # df 1
        (g, 1),                                                  # df 2
        (np.setdiff1d(every, [17]), _geo),                       # df N - 1
        (every, 1),                                              # df N
        (np.union1d(g, rng.choice(n, n // 2 + 10, replace=False)), flag_tf),  # df / N >= 0.5: flagged, tf 9 / 10
        (np.union1d(g, rng.choice(n, 3000, replace=False)), lambda r, d: np.where(np.isin(d, g), 65535, 1 + r.geometric(0.4, len(d))).astype(np.uint16)),
        (np.union1d(g, rng.choice(n, 200, replace=False)), 2),
        (np.union1d(g, rng.choice(n, 20000, replace=False)), _geo),
    ]
    for _ in range(26):  # filler terms: 32-term unions
        specs.append((float(rng.choice([0.0005, 0.003, 0.02, 0.1])), _geo))
    specs.append((np.union1d([4095], rng.choice(n, 60, replace=False)), 1))
    return _gen(n, dl, specs, seed + 1)


@pytest.fixture(scope="module")
def giant_low(S, N):
    c = _giant_corpus(48, 2.0 ** -14, 2.0 ** -13, 11)
    assert 2.0 ** -14 <= _weight_tf1(c.doclen, 4095) < 2.0 ** -13
    sh = S.Shard(0)
    assert _try_upload(S, N, sh, c), "a weight inside the code's range must be accepted"
    yield c, sh
    sh.close()


def test_giant_doc_lowest_binade(S, N, giant_low):
    """the giant doc's weights sit in [2^-14, 2^-13): the 16-bit scan's denormal fold, every kernel family against the exact scores"""
    c, sh = giant_low
    qs = _std_queries(np.random.default_rng(5), len(c.lists), [0, 1, 5, 6])
    _run_all(S, N, sh, c, qs)


def test_giant_doc_tombstones_and_sparse_tier(S, N, giant_low):
    """tombstones (the giant doc among them), then a sparse-tier term found in the giant doc"""
    c, sh = giant_low
    rng = np.random.default_rng(6)
    dele = np.sort(np.concatenate([[4095], rng.choice(c.n_docs, 500, replace=False)]))
    dele = np.unique(dele)
    sh.set_deleted(dele)
    try:
        qs = [([0], False, ()), ([1], False, ()), ([1, 6], False, ()), ([6, 7], True, ()), ([5, 6, 7], False, (1,)), ([3, 4], True, (0,))]
        _run_all(S, N, sh, c, qs, deleted=dele, ks=(1, 10, 129, 1500))
    finally:
        sh.set_deleted([])
    # the sparse tier: one rare term in both giant docs and a few others
    sd = np.array(sorted({4095, c.n_docs - 1, 5, 77, 90000}), np.uint32)
    st = np.array([1, 1, 3, 1, 2], np.uint16)
    first = sh.append_sparse(np.array([0, len(sd)], np.uint64), sd, st)
    assert first == len(c.lists)
    c2 = Corpus(c.n_docs, c.doclen, c.lists + [(sd, st)])
    qs = [([first], False, ()), ([first, 1], False, ()), ([first, 6], True, ()), ([first, 0, 7], False, ())]
    _run_all(S, N, sh, c2, qs, ks=(1, 10, 1500), strategies=(N.BM25_AUTO, N.BM25_EXHAUSTIVE))


def test_giant_doc_out_of_range_is_refused(S, N):
    """the giant doc's weight lies below 2^-14: the upload refuses the image (SS_ENOTSUP); where it is accepted, the answers must be exact"""
    c = _giant_corpus(48, 4.0e-5, 5.6e-5, 12)
    assert _weight_tf1(c.doclen, 4095) < 2.0 ** -14
    sh = S.Shard(0)
    try:
        if _try_upload(S, N, sh, c):
            _run_all(S, N, sh, c, [([0], False, ()), ([1], False, ()), ([1, 6], False, ()), ([6, 7], True, ())], ks=(1, 10, 1500))
    finally:
        sh.close()


@pytest.mark.parametrize("n_text", [6, 40])
def test_mostly_empty(S, N, n_text):
    """length byte 0 for almost every doc; text docs at 0, 4095, 4096, 65535, 65536, n_docs - 1 (and more for n_text = 40): with 6 texts
    of 2000 words their weights have no code (refused), with 40 they do"""
    rng = np.random.default_rng(20 + n_text)
    n = 4096 * 64 + 1
    dl = np.zeros(n, np.uint8)
    texts = np.array([0, 4095, 4096, 65535, 65536, n - 1])
    if n_text > 6:
        texts = np.union1d(texts, rng.choice(n, n_text - 6, replace=False))
    dl[texts] = _b4(2000)[0]
    specs = [(texts, 1), (texts, 2), (texts[::2], 3), (np.union1d(texts, rng.choice(n, 5000, replace=False)), 1),
             (np.union1d(texts[:3], rng.choice(n, 100, replace=False)), _geo), (float(0.2), _geo)]
    c = _gen(n, dl, specs, 3)
    sh = S.Shard(0)
    try:
        ok = _try_upload(S, N, sh, c)
        if n_text > 6:
            assert ok, "weights inside the code's range must be accepted"
        if ok:
            qs = [([0], False, ()), ([1], False, ()), ([0, 1], False, ()), ([0, 1], True, ()), ([2, 3, 4], False, ()),
                  ([3, 5], True, ()), ([0, 3, 4, 5], False, (2,)), ([1, 3], True, (4,))]
            _run_all(S, N, sh, c, qs, ks=(1, 10, 129, 1500))
    finally:
        sh.close()


def test_exact_ties_in_doc_order(S, N):
    """one length, tf = 1: every score of a query is bit-equal, across many sub-blocks and probe partitions -- the top k must be the
    k lowest matching doc ids, exactly"""
    rng = np.random.default_rng(31)
    n = 4096 * 40
    dl = np.full(n, _b4(100)[0], np.uint8)
    specs = [(0.3, 1), (0.05, 1), (0.6, 1), (0.002, 1), (np.arange(0, n, 7), 1)]
    c = _gen(n, dl, specs, 4)
    sh = S.Shard(0)
    try:
        assert _try_upload(S, N, sh, c)
        qs = [([0], False, ()), ([1], False, ()), ([2], False, ()), ([4], False, ()), ([0, 2], True, ()), ([1, 3], True, ()),
              ([0, 4], True, ()), ([3], False, ())]
        _run_all(S, N, sh, c, qs, exact_ties=True)
    finally:
        sh.close()


def test_three_fields_one_long_field(S, N, O):
    """three indexed fields, one field of one doc the long one: its per-field weight has no code -- refused, or answered exactly"""
    rng = np.random.default_rng(41)
    n, F = 4096 * 12, 3
    dlf = np.stack([_b4(rng.integers(5, 40, n)) for _ in range(F)])
    dlf[1, 4095] = 0
    dlf[1, 4095] = 255  # (SmallFloat's largest length: far beyond 4 10^4 times the fields' average)
    offs, docs, fields, tfs = [0], [], [], []
    for t in range(6):
        dd = np.union1d([4095], rng.choice(n, 2000 * (t + 1), replace=False))
        for d in dd:
            fs = [1] if d == 4095 else sorted(rng.choice(F, int(rng.integers(1, F + 1)), replace=False).tolist())
            for f in fs:
                docs.append(d); fields.append(f); tfs.append(int(rng.integers(1, 5)))
        offs.append(len(docs))
    offs = np.array(offs, np.uint64)
    docs, fields, tfs = np.array(docs, np.uint32), np.array(fields, np.uint8), np.array(tfs, np.uint16)
    boost = np.array([1.0, 1.5, 0.7], np.float32)
    sh = S.Shard(0)
    try:
        try:
            sh.upload_lexical_fields(n, dlf, boost, offs, docs, fields, tfs)
        except N.SeekStormHipError as e:
            assert e.code == N.SS_ENOTSUP, e
            return
        for terms, qt, op in (([0], S.QueryType.Union, O.OP_OR), ([0, 3], S.QueryType.Intersection, O.OP_AND),
                              ([1, 2, 5], S.QueryType.Union, O.OP_OR)):
            q = sh.make_queries([terms], qt)
            for k in (100, 2500):  # (2500: every match of the first two, the long field's doc at the bottom)
                d, s, cnt, tot = sh.search_lexical_batch(q, k, S.ResultType.TopkCount, reference_shortcuts=False)
                od, os_, otot, _ = O.search_fields_exhaustive(n, dlf, boost, offs, docs, fields, tfs, terms, op, k)
                assert int(tot[0]) == otot and int(cnt[0]) == len(od)
                assert np.allclose(s[0][:len(od)], os_, rtol=REL), f"fields {terms} k={k}: scores off by {np.max(np.abs(s[0][:len(od)] / os_ - 1)):.3g}"
    finally:
        sh.close()


def test_commit_pushes_postings_out_of_range(S, N):
    """levels without the giant doc, then one holding it (inside the code: accepted, the whole re-coded image checked), then a level of
    empty docs that lowers avgdl and pushes the giant doc's postings below 2^-14: refused, the previous image and levels stay"""
    rng = np.random.default_rng(51)
    L = 65536
    n_all = 4 * L
    dl = _b4(rng.integers(10, 31, n_all))
    dl[3 * L:] = 0  # level 3: empty docs
    giant = 2 * L + 4095
    lists_all = []
    for t in range(6):
        dd = np.union1d([giant], rng.choice(3 * L, 1500 * (t + 1), replace=False)) if t < 4 else rng.choice(n_all, 3000, replace=False)
        dd = np.unique(dd).astype(np.uint32)
        lists_all.append((dd, np.where(dd == giant, 1, 1 + rng.geometric(0.5, len(dd))).astype(np.uint16)))
    # the giant doc's length: inside the code once three levels are in, outside once the empty level joins
    dl3 = dl[:3 * L].copy()
    dl[giant] = _len_for_ratio(dl3, giant, 2.0 ** -14, 2.0 ** -13)
    assert 2.0 ** -14 <= _weight_tf1(dl[:3 * L], giant)
    assert _weight_tf1(dl, giant) < 2.0 ** -14

    def level(lv):
        lo, hi = lv * L, (lv + 1) * L
        offs, docs, tfs = [0], [], []
        for d, t in lists_all:
            m = (d >= lo) & (d < hi)
            docs.append(d[m]); tfs.append(t[m]); offs.append(offs[-1] + int(m.sum()))
        return np.array(offs, np.uint64), np.concatenate(docs), np.concatenate(tfs)

    sh = S.Shard(0)
    try:
        for lv in range(3):
            o, d, t = level(lv)
            sh.append_level(lv, dl[lv * L:(lv + 1) * L], o, d, t)
        c = Corpus(3 * L, dl[:3 * L], [(d[d < 3 * L], t[d < 3 * L]) for d, t in lists_all])
        qs = [([0], False, ()), ([0, 1], False, ()), ([0, 1], True, ()), ([2, 3, 4], False, ()), ([0, 5], False, (3,))]
        _run_all(S, N, sh, c, qs, ks=(1, 10, 129, 1500), strategies=(N.BM25_AUTO, N.BM25_EXHAUSTIVE, N.BM25_PRUNED))
        o, d, t = level(3)
        try:
            sh.append_level(3, dl[3 * L:], o, d, t)
            accepted = True
        except N.SeekStormHipError as e:
            assert e.code == N.SS_ENOTSUP, e
            accepted = False
        if accepted:  # (then the four-level image must be exact)
            c4 = Corpus(n_all, dl, lists_all)
            _run_all(S, N, sh, c4, qs, ks=(1, 10, 1500), strategies=(N.BM25_AUTO, N.BM25_EXHAUSTIVE))
        else:
            assert sh.incremental_info()[0] == 3
            _run_all(S, N, sh, c, qs, ks=(1, 10, 1500), strategies=(N.BM25_AUTO, N.BM25_EXHAUSTIVE))
    finally:
        sh.close()


# ---------------------------------------------------------------- phrases naming unique terms past slot 11
def _phrase_corpus(O, seed):
    rng = np.random.default_rng(seed)
    n = 4096 * 2 + 1
    n_terms = 24
    lens = rng.integers(30, 60, n)
    dl = _b4(lens)
    # every doc: a random text over the 24 terms; docs 0..299 hold the phrase "t12 t13 ... t19" at a random place
    texts = [rng.integers(0, n_terms, int(x)) for x in lens]
    for d in range(300):
        at = int(rng.integers(0, len(texts[d]) - 8))
        texts[d][at:at + 8] = np.arange(12, 20)
    for d in range(300, 600):  # near misses: the words out of order
        at = int(rng.integers(0, len(texts[d]) - 8))
        texts[d][at:at + 8] = np.arange(19, 11, -1)
    offs, docs, tfs, pos = [0], [], [], []
    for t in range(n_terms):
        for d in range(n):
            p = np.nonzero(texts[d] == t)[0]
            if len(p):
                docs.append(d); tfs.append(len(p)); pos.extend(p.tolist())
        offs.append(len(docs))
    return n, dl, np.array(offs, np.uint64), np.array(docs, np.uint32), np.array(tfs, np.uint16), np.array(pos, np.uint16)


def test_phrase_seq_past_twelve_slots(S, N, O):
    """raw queries of 13..20 unique terms whose phrase words name terms 12..19 (with and without SS_PHRASE_SKIP places): the answer
    equals the oracle's phrase search, or the batch is refused with SS_ENOTSUP -- never a wrong answer, never SS_EINVAL"""
    import torch
    n, dl, offs, docs, tfs, pos = _phrase_corpus(O, 61)
    sh = S.Shard(0)
    osh = O.Shard(n, dl, offs, docs, tfs)
    osh.set_positions(pos)
    try:
        sh.upload_lexical(n, dl, offs, docs, tfs, positions=pos)
        cases = []
        for nt in (13, 16, 20):
            terms = list(range(nt))
            for skip in (False, True):
                seq = list(range(max(10, nt - 8), nt))  # words naming terms 12 .. 19 (and 10, 11 before them)
                if skip:
                    seq = [seq[0], N.SS_PHRASE_SKIP] + seq[2:]
                cases.append((terms, seq))
        qs = np.zeros(len(cases), N.BM25_QUERY_DTYPE)
        for i, (terms, seq) in enumerate(cases):
            qs["n_terms"][i] = len(terms)
            qs["op"][i] = int(S.QueryType.Phrase)
            for j, t in enumerate(terms):
                qs["term"][i, j] = t
                qs["idf"][i, j] = S.idf_f32(n, int(offs[t + 1] - offs[t]))
            qs["phrase_len"][i] = len(seq)
            qs["phrase_seq"][i, :len(seq)] = seq
        for k in (10, 200):
            for batch in ("host", "dev"):
                try:
                    if batch == "host":
                        d, s, cnt, tot = sh.search_lexical_batch(qs, k, S.ResultType.TopkCount, reference_shortcuts=False)
                    else:
                        dev = torch.device("cuda", 0)
                        nq = len(qs)
                        qd = torch.from_numpy(qs.view(np.uint8).reshape(nq, -1).copy()).to(dev)
                        dd = torch.full((nq, k), -1, dtype=torch.int32, device=dev)
                        ds = torch.zeros((nq, k), dtype=torch.float32, device=dev)
                        dc = torch.zeros((nq,), dtype=torch.int32, device=dev)
                        dt = torch.zeros((nq,), dtype=torch.int64, device=dev)
                        N.check(N.lib().ss_bm25_search_dev(sh._h, nq, qd.data_ptr(), k, int(S.ResultType.TopkCount), 16 | (20 << 8), dd.data_ptr(),
                                                           ds.data_ptr(), dc.data_ptr(), dt.data_ptr(), None), "ss_bm25_search_dev")
                        torch.cuda.synchronize()
                        d, s, cnt, tot = dd.cpu().numpy().view(np.uint32), ds.cpu().numpy(), dc.cpu().numpy(), dt.cpu().numpy()
                except N.SeekStormHipError as e:
                    assert e.code == N.SS_ENOTSUP, e
                    continue
                for i, (terms, seq) in enumerate(cases):
                    if N.SS_PHRASE_SKIP in seq:  # an n-gram key at place 0: its entry, then the words behind it
                        places = [j for j, x in enumerate(seq) if x != N.SS_PHRASE_SKIP]
                        od, os_, otot = osh.search_phrase_items(terms, [seq[j] for j in places], places, k)
                    else:
                        od, os_, otot = osh.search_phrase(terms, seq, k)
                    where = f"{batch} k={k} {len(terms)} terms seq {seq}"
                    assert int(tot[i]) == otot, f"{where}: {int(tot[i])} matches, want {otot}"
                    assert int(cnt[i]) == len(od), where
                    assert np.allclose(s[i][:len(od)], os_, rtol=REL), where
    finally:
        sh.close()


def test_phrase_through_giant_doc(S, N, O):
    """a phrase whose matches include a giant doc in the code's lowest binade: the phrase kernels against the oracle"""
    rng = np.random.default_rng(71)
    n = 4096 * 12 + 1
    lens = rng.integers(10, 31, n)
    dl = _b4(lens)
    giant = 4095
    dl[giant] = _len_for_ratio(dl, giant, 2.0 ** -14, 2.0 ** -13)
    # terms 0, 1: the phrase "0 1" in the giant doc and in docs 100..199; term 2 elsewhere
    per = {0: {}, 1: {}, 2: {}}
    for d in list(range(100, 200)) + [giant]:
        per[0][d] = [3]; per[1][d] = [4]
    for d in range(200, 260):
        per[0][d] = [5]; per[1][d] = [2]
    for d in rng.choice(n, 400, replace=False):
        per[2][int(d)] = [1]
    offs, docs, tfs, pos = [0], [], [], []
    for t in range(3):
        for d in sorted(per[t]):
            docs.append(d); tfs.append(len(per[t][d])); pos.extend(per[t][d])
        offs.append(len(docs))
    offs, docs, tfs, pos = np.array(offs, np.uint64), np.array(docs, np.uint32), np.array(tfs, np.uint16), np.array(pos, np.uint16)
    sh = S.Shard(0)
    osh = O.Shard(n, dl, offs, docs, tfs)
    osh.set_positions(pos)
    try:
        sh.upload_lexical(n, dl, offs, docs, tfs, positions=pos)
        q = sh.make_queries([[0, 1]], S.QueryType.Phrase)
        for k in (1, 10, 200):
            d, s, cnt, tot = sh.search_lexical_batch(q, k, S.ResultType.TopkCount, reference_shortcuts=False)
            od, os_, otot = osh.search_phrase([0, 1], [0, 1], k)
            assert int(tot[0]) == otot == 101 and int(cnt[0]) == len(od)
            assert np.allclose(s[0][:len(od)], os_, rtol=REL)
            assert giant in set(int(x) for x in d[0][:cnt[0]]) or k < 101
    finally:
        sh.close()
