"""ss_bm25_commit_sparse_level_fields beside ss_bm25_commit_level_fields: an image with several indexed fields AND a sparse tier that
grows level by level.  Per commit the dense terms' entries go through the dense commit and the rare terms' entries through the sparse
one; the tier keeps one merged posting per (term, doc) with the tf of every field and is re-coded on the device whenever avgdl and the
merged lists' scale move.  After every step the shard must answer exactly (np.array_equal) like a fresh shard that got ONE
upload_lexical_fields of the prefix's dense terms plus ONE append_sparse_fields of its rare terms.  A level is 65 536 docs, so the corpus
is two full levels and a partial third, with small dfs."""
import ctypes as C
import os

import numpy as np
import pytest

from test_gpu_commit_fields import Corpus, _edit, _answer, _refused, _same_result, _b4

pytestmark = pytest.mark.gpu

LVL = 65536
N_DOCS = 2 * LVL + 30_000
PARTIAL = 12_000          # docs of level 2 when it is first committed
BOOST = [2.0, 1.0, 0.5]
ND = 6                    # dense terms 0..5, rare terms 6..9
#        0      1      2      3      4    5 (nobody's)  6    7   8   9 (known from the last step on)
DFS = [9_000, 6_000, 12_000, 3_000, 4_000, 0, 400, 900, 60, 200]
EMPTY, ABSENT_L1, ONE_FIELD, EDGES, LATE = 5, 6, 7, 8, 9
# (level, first doc, end doc, terms known)
STEPS = [(0, 0, LVL, 9), (1, LVL, 2 * LVL, 9), (2, 2 * LVL, 2 * LVL + PARTIAL, 9), (2, 2 * LVL, N_DOCS, 10)]
EDGE_DOCS = [0, 4095, 4096, LVL - 1, LVL, 2 * LVL - 1, 2 * LVL, 2 * LVL + PARTIAL - 1, N_DOCS - 1]


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


@pytest.fixture(scope="module")
def corpus(O):
    from test_gpu_phrase import _corpus_fields
    plant = [([0, 1], 0, 300), ([0, 1], 2, 200), ([3, 4], 2, 60), ([6, 0], 0, 80), ([1, 6], 2, 80)]
    cross = [(0, 1, 500), (6, 0, 60)]
    dl, offs, docs, fields, tfs, positions = _corpus_fields(O, N_DOCS, 3, DFS, 29, plant, cross)
    planted = {}

    def edit(terms):
        terms[ABSENT_L1] = {k: v for k, v in terms[ABSENT_L1].items() if not LVL <= k[0] < 2 * LVL}
        terms[ONE_FIELD] = {k: v for k, v in terms[ONE_FIELD].items() if k[1] == 1}
        terms[LATE] = {k: v for k, v in terms[LATE].items() if k[0] >= 2 * LVL + PARTIAL}  # (only the re-committed level has seen it)
        for d in EDGE_DOCS:  # postings on the first and the last doc of a sub-block, of a level, of the partial level and of the corpus
            terms[EDGES].setdefault((d, 1), [3, 9])
        terms[EDGES][(4096, 0)] = [1]; terms[EDGES][(4096, 2)] = [2, 5, 8]  # ... and one doc with the term in all three fields
        # a rare word next to a dense one: how many docs hold the phrase in the planted field
        planted["6 0 in field 0"] = sum(1 for (d, f), ps in terms[6].items() if f == 0 and any(p + 1 in terms[0].get((d, 0), []) for p in ps))
        planted["1 6 in field 2"] = sum(1 for (d, f), ps in terms[1].items() if f == 2 and any(p + 1 in terms[6].get((d, 2), []) for p in ps))

    offs, docs, fields, tfs, positions = _edit(offs, docs, fields, tfs, positions, edit)
    c = Corpus(dl, offs, docs, fields, tfs, positions)
    # what the corpus must hold, so that nothing below passes vacuously
    of = lambda t: slice(int(offs[t]), int(offs[t + 1]))
    assert offs[EMPTY] == offs[EMPTY + 1]
    assert not np.any((docs[of(ABSENT_L1)] >= LVL) & (docs[of(ABSENT_L1)] < 2 * LVL)) and np.any(docs[of(ABSENT_L1)] < LVL)
    assert np.any(docs[of(ABSENT_L1)] >= 2 * LVL)
    assert set(fields[of(ONE_FIELD)].tolist()) == {1} and len(docs[of(ONE_FIELD)]) > 100
    for d in EDGE_DOCS:
        assert d in docs[of(EDGES)]
    assert np.sum(docs[of(EDGES)] == 4096) == 3
    assert offs[LATE + 1] - offs[LATE] >= 10 and docs[of(LATE)].min() >= 2 * LVL + PARTIAL
    assert planted["6 0 in field 0"] >= 30 and planted["1 6 in field 2"] >= 30, planted
    for t in range(ND, 10):  # every rare list: far below the dense ones
        assert len(np.unique(docs[of(t)])) < 1100
    c.planted = planted
    return c


SETS = [[0, 1], [1, 2, 3], [0, 6], [1, 6, 4], [8, 0], [7, 2], [5, 0], [9, 1], [8], [6, 7], [2, 3], [7], [6, 8, 7], [6]]
NOTS = [[], [4], [], [2], [], [1], [], [], [7], [], [6], [8], [0], []]
PHRASES = [[0, 1], [1, 0], [6, 0], [0, 6], [1, 6], [6, 1], [3, 4], [7, 2]]


def _queries(S, sh, nt, positions):
    """(name, query array) of the whole query set over the terms known so far"""
    use = [(l, n) for l, n in zip(SETS, NOTS) if max(l + n) < nt]
    out = []
    for qt in (S.QueryType.Union, S.QueryType.Intersection):
        out.append((("sets", qt), sh.make_queries([u[0] for u in use], qt)))
        out.append((("NOT terms", qt), sh.make_queries([u[0] for u in use], qt, [u[1] for u in use])))
    for ff in ([1], [0, 2]):
        out.append((("filtered intersections", tuple(ff)), sh.make_queries([u[0] for u in use], S.QueryType.Intersection, field_filter=ff)))
    if positions:
        out.append((("phrases",), sh.make_queries(PHRASES, S.QueryType.Phrase)))
        out.append((("phrases in field 1",), sh.make_queries(PHRASES, S.QueryType.Phrase, field_filter=[1])))
        out.append((("phrases in fields 0, 2",), sh.make_queries(PHRASES, S.QueryType.Phrase, field_filter=[0, 2])))
    return out


def _all_answers(S, N, sh, nt, positions):
    return {(name, k, rt): _answer(N, sh, q, k, rt) for name, q in _queries(S, sh, nt, positions)
            for k in (10, 100) for rt in (S.ResultType.TopkCount, S.ResultType.Count)}


def _compare(S, N, inc, one, nt, positions, what):
    assert inc.fields_info() == one.fields_info(), what
    assert inc.sparse_info()[:2] == one.sparse_info()[:2] == (nt - ND, inc.sparse_info()[1]), (what, inc.sparse_info(), one.sparse_info())
    terms = np.arange(nt, dtype=np.uint32)
    assert np.array_equal(inc.posting_count(terms), one.posting_count(terms)), what
    for (name, qi), (_, qo) in zip(_queries(S, inc, nt, positions), _queries(S, one, nt, positions)):
        assert np.array_equal(qi.view(np.uint8), qo.view(np.uint8)), ("idf differs: the two images disagree on N or df", what, name)
    a, b = _all_answers(S, N, inc, nt, positions), _all_answers(S, N, one, nt, positions)
    refused = [(key, b[key]) for key in b if _refused(b[key])]
    assert not refused, ("the one-shot shard must answer the whole set", what, refused)
    for key in a:
        _same_result(a[key], b[key], (what, key))
    return a


def _split(level):
    """a level's CSR of all known terms -> (doclen, dense call's arrays, rare call's arrays), as Shard.commit_level_fields_tiered cuts it"""
    ldl, lo_, ld, lf, lt, lp = level
    cut = int(lo_[ND])
    p_cut = int(lt[:cut].astype(np.int64).sum())
    return ldl, (lo_[:ND + 1], ld[:cut], lf[:cut], lt[:cut], lp[:p_cut]), (lo_[ND:] - lo_[ND], ld[cut:], lf[cut:], lt[cut:], lp[p_cut:])


def _commit_dense(sh, lv, ldl, dense, positions, boost=BOOST):
    sh.commit_level_fields(lv, ldl, boost, *dense[:4], positions=dense[4] if positions else None)


def _commit_rare(sh, lv, rare, positions):
    sh.commit_sparse_level_fields(lv, *rare[:4], positions=rare[4] if positions else None)


def _commit(sh, c, step, positions, tiered_call=False):
    lv, lo, hi, nt = step
    level = c.level(lo, hi, nt)
    if tiered_call:
        ldl, lo_, ld, lf, lt, lp = level
        sh.commit_level_fields_tiered(lv, ldl, BOOST, lo_, ld, lf, lt, ND, positions=lp if positions else None)
        return
    ldl, dense, rare = _split(level)
    _commit_dense(sh, lv, ldl, dense, positions)
    _commit_rare(sh, lv, rare, positions)


def _upload(one, c, hi, nt, positions, boost=BOOST):
    """ONE upload of the prefix's dense terms plus ONE append of its rare terms"""
    pdl, dense, rare = _split(c.prefix(hi, nt))
    one.upload_lexical_fields(hi, pdl, boost, *dense[:4], dense[4] if positions else None)
    assert one.append_sparse_fields(*rare[:4], positions=rare[4] if positions else None) == ND


def _oracle(S, O, c, sh):
    pdl, po, pd, pf, pt, pp = c.prefix(N_DOCS, 10)
    for terms, qt, op in (([6, 1], S.QueryType.Union, O.OP_OR), ([2, 7], S.QueryType.Intersection, O.OP_AND)):
        d, s, cnt, tot = sh.search_lexical_batch(sh.make_queries([terms], qt), 10, reference_shortcuts=False)
        od, os_, otot, _ = O.search_fields_exhaustive(N_DOCS, pdl, BOOST, po, pd, pf, pt, terms, op, 10)
        assert otot > 0 and int(tot[0]) == otot and int(cnt[0]) == len(od) and np.allclose(s[0][:len(od)], os_, rtol=1e-4), terms


@pytest.mark.parametrize("positions", [True, False])
def test_tiered_commits_equal_one_upload_plus_one_append(S, N, O, corpus, positions):
    """levels 0 and 1, a partial level 2, level 2 re-committed whole with a rare term no level had seen (the tier grows by a list): after
    every step the same fields_info, sparse lists and postings, posting counts, query records (idf), and bit-equal answers -- unions and
    intersections mixing dense and rare terms, NOT terms of either tier, field filters, phrases naming a rare word with and without a
    field filter, k 10 and 100, TopkCount and Count; two queries against the oracle.  Without positions a phrase raises on both shards."""
    inc, one = S.Shard(0), S.Shard(0)
    try:
        for step in STEPS:
            _commit(inc, corpus, step, positions)
            _upload(one, corpus, step[2], step[3], positions)
            assert inc.fields_info() == (3, True, positions)
            a = _compare(S, N, inc, one, step[3], positions, step)
            n_lists, n_post, n_bytes = inc.sparse_info()
            assert n_bytes == n_post * (8 + 2 * 3) + (n_lists + 1) * 8  # the tf of every field beside a posting
            assert inc.incremental_info()[0] == step[0] + 1
        _oracle(S, O, corpus, inc)
        if positions:  # the planted phrases are found, in their field only
            tot = {name: a[(name, 10, S.ResultType.TopkCount)][3] for name in (("phrases",), ("phrases in field 1",), ("phrases in fields 0, 2",))}
            i60, i16 = PHRASES.index([6, 0]), PHRASES.index([1, 6])
            assert int(tot[("phrases",)][i60]) >= corpus.planted["6 0 in field 0"] >= 30 and int(tot[("phrases",)][i16]) >= corpus.planted["1 6 in field 2"] >= 30
            assert int(tot[("phrases in fields 0, 2",)][i60]) >= 30 and int(tot[("phrases in field 1",)][i60]) < int(tot[("phrases",)][i60])
        else:
            for sh in (inc, one):
                with pytest.raises(N.SeekStormHipError):
                    sh.search_lexical_batch(sh.make_queries([[6, 0]], S.QueryType.Phrase), 10)
        assert int(inc.posting_count(np.array([EMPTY], np.uint32))[0]) == 0 and int(inc.posting_count(np.array([LATE], np.uint32))[0]) >= 10
    finally:
        inc.close(); one.close()


def test_commit_level_fields_tiered_gives_the_same_image(S, N, corpus):
    """the same steps through Shard.commit_level_fields_tiered (one CSR of all terms, split where the dense terms end) answer like the
    two explicit calls per step"""
    two, one_call = S.Shard(0), S.Shard(0)
    try:
        for step in STEPS:
            _commit(two, corpus, step, True)
            _commit(one_call, corpus, step, True, tiered_call=True)
        assert two.fields_info() == one_call.fields_info() and two.sparse_info() == one_call.sparse_info() == (4, two.sparse_info()[1], two.sparse_info()[2])
        a, b = _all_answers(S, N, two, 10, True), _all_answers(S, N, one_call, 10, True)
        for key in a:
            assert not _refused(a[key]), key
            _same_result(a[key], b[key], key)
    finally:
        two.close(); one_call.close()


def _merged_scale(c, hi, nt):
    """the merged lists' scale of the prefix's DENSE terms as the builders choose it: the power of two above (largest merged weight) / 3.99"""
    pdl, po, pd, pf, pt, _ = c.prefix(hi, nt)
    cut = int(po[ND])
    table = np.array([_b4(b) for b in range(256)], np.float32)
    avgdl = np.float32(table[pdl].astype(np.float64).sum() / hi)
    ln = table[pdl[pf[:cut].astype(np.int64), pd[:cut].astype(np.int64)]]
    comp = np.float32(1.2) * (np.float32(0.25) + np.float32(0.75) * (ln / avgdl))
    tf = pt[:cut].astype(np.float32)
    part = np.asarray(BOOST, np.float32)[pf[:cut]] * (tf * np.float32(2.2) / (tf + comp))
    et = np.repeat(np.arange(ND), np.diff(po[:ND + 1].astype(np.int64)))
    w = np.bincount(et.astype(np.int64) * hi + pd[:cut], weights=part.astype(np.float64))
    return float(2.0 ** np.frexp(w.max() / 3.99)[1]), float(w.max())


@pytest.fixture(scope="module")
def scale_corpus(O):
    """level 0: 65 536 docs whose terms stand in field 2 only (boost 0.5), with tf 1; level 1: 3000 docs that hold dense term 0 in
    all three fields with tf 12 -- the largest merged weight, and with it the merged lists' scale, jumps with level 1"""
    rng = np.random.default_rng(5)
    n = LVL + 3000
    dl = np.stack([O.lex_doclen(n, seed=O.LEX_SEED + 7 * f) for f in range(3)])
    ent = [[] for _ in range(ND + 2)]  # per term (doc, field, tf)
    for t, df in ((0, 3000), (1, 2000), (2, 1500), (3, 800), (4, 500)):
        ent[t] += [(int(d), 2, 1) for d in rng.choice(LVL, df, replace=False)]
    ent[0] += [(int(d), f, 12) for d in range(LVL + 100, LVL + 600) for f in range(3)]
    ent[1] += [(int(d), 2, 1) for d in range(LVL + 300, LVL + 900)]
    for t, df0, df1 in ((ND, 150, 40), (ND + 1, 60, 25)):
        # the rare terms: in level 0 like the dense ones (their weights must fit the scale the dense lists chose, or the level is
        # refused like the one-shot append), in level 1 in one or two fields
        ent[t] += [(int(d), 2, 1) for d in rng.choice(LVL, df0, replace=False)]
        for d in LVL + rng.choice(3000, df1, replace=False):
            ent[t].append((int(d), int(d) % 3, 1 + int(d) % 4))
            if d % 5 == 0:
                ent[t].append((int(d), (int(d) + 1) % 3, 2))
    offs, docs, fields, tfs = [0], [], [], []
    for e in ent:
        for d, f, tf in sorted(e):
            docs.append(d); fields.append(f); tfs.append(tf)
        offs.append(len(docs))
    tfs = np.asarray(tfs, np.uint16)
    pos = np.concatenate([np.arange(t, dtype=np.uint16) * 3 + 1 for t in tfs])
    return Corpus(dl, np.asarray(offs, np.uint64), np.asarray(docs, np.uint32), np.asarray(fields, np.uint8), tfs, pos)


def test_the_tier_follows_a_moving_merged_scale(S, N, scale_corpus):
    """level 1's dense postings move the merged lists' scale (asserted on the host from the two prefixes): right after the dense commit
    the tier's older postings are re-coded against the new scale and average length -- rare terms score like a one-shot image of the
    new dense prefix with the OLD rare postings --, and after the sparse commit like the one-shot image of the whole prefix"""
    c, nt, n = scale_corpus, ND + 2, LVL + 3000
    s0, w0 = _merged_scale(c, LVL, nt)
    s1, w1 = _merged_scale(c, n, nt)
    assert s0 != s1 and w0 < 1.2 and w1 > 5.0, (s0, w0, s1, w1)
    inc, one = S.Shard(0), S.Shard(0)
    try:
        q_of = lambda sh: sh.make_queries([[ND], [ND + 1], [ND, 0], [ND + 1, ND], [1, ND]], S.QueryType.Union)
        ans = lambda sh: _answer(N, sh, q_of(sh), 100, S.ResultType.TopkCount)
        ldl, dense, rare = _split(c.level(0, LVL, nt))
        _commit_dense(inc, 0, ldl, dense, True)
        _commit_rare(inc, 0, rare, True)
        _upload(one, c, LVL, nt, True)
        before = ans(inc)
        _same_result(before, ans(one), "level 0")
        ldl, dense, rare1 = _split(c.level(LVL, n, nt))
        _commit_dense(inc, 1, ldl, dense, True)
        # the one-shot image of the new dense prefix with the rare postings of level 0 only
        pdl, pdense, _ = _split(c.prefix(n, nt))
        _, _, prare0 = _split(c.prefix(LVL, nt))
        one.upload_lexical_fields(n, pdl, BOOST, *pdense)
        assert one.append_sparse_fields(*prare0[:4], positions=prare0[4]) == ND
        between = ans(inc)
        _same_result(between, ans(one), "between the dense and the sparse commit of level 1")
        assert not _refused(between) and not np.array_equal(between[1], before[1])  # (the scores moved with avgdl)
        _commit_rare(inc, 1, rare1, True)
        _upload(one, c, n, nt, True)
        after = ans(inc)
        _same_result(after, ans(one), "level 1")
        assert inc.sparse_info()[:2] == one.sparse_info()[:2] and int(after[3][0]) > int(between[3][0])
    finally:
        inc.close(); one.close()


def test_entry_codes_and_atomicity(S, N, corpus):
    """every refusal of the sparse commit, of the dense commit beside a tier of levels and of the whole-list append on such a tier: the
    code, and afterwards the same answers of a fixed query set and the same sparse_info"""
    hi = LVL + 20_000
    l0 = _split(corpus.level(0, LVL, 9))
    l1 = _split(corpus.level(LVL, hi, 9))
    q_sets = [[0, 1], [6, 0], [8], [7, 2], [6, 7]]

    def state(sh):
        return (sh.sparse_info()[:2], _answer(N, sh, sh.make_queries(q_sets, S.QueryType.Union), 10, S.ResultType.TopkCount),
                _answer(N, sh, sh.make_queries([[6, 0], [0, 1]], S.QueryType.Phrase), 10, S.ResultType.TopkCount))

    def same(a, b, what):
        assert a[0] == b[0], what
        _same_result(a[1], b[1], what); _same_result(a[2], b[2], what)
        assert not _refused(a[1]) and not _refused(a[2]), what

    def code_of(call):
        with pytest.raises(N.SeekStormHipError) as e:
            call()
        return e.value.code

    inc, one = S.Shard(0), S.Shard(0)
    try:
        assert code_of(lambda: _commit_rare(inc, 0, l0[2], True)) == N.SS_ESTATE  # a shard with no image
        _commit_dense(inc, 0, l0[0], l0[1], True)
        _commit_rare(inc, 0, l0[2], True)
        dq = lambda sh: _answer(N, sh, sh.make_queries([[0, 1], [1, 2, 3], [4]], S.QueryType.Union, [[], [4], []]), 100, S.ResultType.TopkCount)
        level0 = dq(inc)
        _commit_dense(inc, 1, l1[0], l1[1], True)
        # dense-only queries answer the new level right away, before its sparse commit arrives
        _upload(one, corpus, hi, 9, True)
        _same_result(dq(inc), dq(one), "dense terms after the dense commit")
        assert not _refused(level0) and np.all(dq(inc)[3] > level0[3])  # (every total grew by the level's docs)
        _commit_rare(inc, 1, l1[2], True)
        good = state(inc)
        same(good, state(one), "two levels")
        o, d, f, t, p = l1[2]
        refusals = [
            ("a level that is not the last committed", lambda: inc.commit_sparse_level_fields(2, o, d, f, t, positions=p), N.SS_EINVAL),
            ("a level older than the tier's last", lambda: _commit_rare(inc, 0, l0[2], True), N.SS_EINVAL),
            ("fewer lists than the tier holds", lambda: inc.commit_sparse_level_fields(1, o[:3], d[:int(o[2])], f[:int(o[2])], t[:int(o[2])],
                                                                                      positions=p[:int(t[:int(o[2])].sum())]), N.SS_EINVAL),
            ("a posting of the level before", lambda: inc.commit_sparse_level_fields(1, o, np.where(np.arange(len(d)) == 0, 17, d).astype(np.uint32),
                                                                                    f, t, positions=p), N.SS_EINVAL),
            ("a posting behind the level's docs", lambda: inc.commit_sparse_level_fields(1, o, np.where(np.arange(len(d)) == len(d) - 1, hi, d).astype(np.uint32),
                                                                                        f, t, positions=p), N.SS_EINVAL),
            ("no positions on an image with positions", lambda: inc.commit_sparse_level_fields(1, o, d, f, t), N.SS_EINVAL),
            ("one position too few", lambda: inc.commit_sparse_level_fields(1, o, d, f, t, positions=p[:-1]), N.SS_EINVAL),
            ("tf 0", lambda: inc.commit_sparse_level_fields(1, o, d, f, np.where(np.arange(len(t)) == 1, 0, t).astype(np.uint16), positions=p[:len(p) - int(t[1])]),
             N.SS_EINVAL),
            ("whole lists on a tier of levels", lambda: inc.append_sparse_fields(o, d, f, t, positions=p), N.SS_ESTATE),
            # the dense commit beside a tier of levels
            ("more dense terms than the image holds", lambda: inc.commit_level_fields(1, l1[0], BOOST, *_dense_terms(corpus, LVL, hi, 7)), N.SS_ENOTSUP),
            ("a shrunk re-commit", lambda: inc.commit_level_fields(1, *_shrunk(corpus, LVL, LVL + 2000)), N.SS_ENOTSUP),
        ]
        assert len(d) >= 10 and d[0] >= LVL and int(t[1]) >= 1
        for what, call, want in refusals:
            assert code_of(call) == want, what
            same(state(inc), good, what)
            assert inc.incremental_info()[0] == 2, what
        # the tier still takes its level: the same level again replaces what it brought
        _commit_rare(inc, 1, l1[2], True)
        same(state(inc), good, "level 1 brought twice")
    finally:
        inc.close(); one.close()
    # positions on an image without
    nop = S.Shard(0)
    try:
        _commit_dense(nop, 0, l0[0], l0[1], False)
        _commit_rare(nop, 0, l0[2], False)
        before = (nop.sparse_info(), _answer(N, nop, nop.make_queries(q_sets, S.QueryType.Union), 10, S.ResultType.TopkCount))
        assert code_of(lambda: _commit_rare(nop, 0, l0[2], True)) == N.SS_EINVAL
        after = (nop.sparse_info(), _answer(N, nop, nop.make_queries(q_sets, S.QueryType.Union), 10, S.ResultType.TopkCount))
        assert before[0] == after[0] and not _refused(before[1])
        _same_result(before[1], after[1], "positions on an image without")
    finally:
        nop.close()
    # images built another way, a tier of whole lists, an image without merged lists
    sdl, sdense, srare = _split(corpus.level(0, 3000, 9))
    m1 = (corpus.fields == 0) & (corpus.docs < 3000) & (corpus.eterm < ND)
    o1 = np.zeros(ND + 1, np.uint64); o1[1:] = np.cumsum(np.bincount(corpus.eterm[m1], minlength=ND)[:ND])
    far = [4096.0, 1.0, 1.0 / 4096.0]
    for what, build, want in (
            ("a one-shot upload", lambda sh: sh.upload_lexical_fields(3000, sdl, BOOST, *sdense), N.SS_ESTATE),
            ("one-field levels", lambda sh: sh.append_level(0, corpus.dl[0, :3000], o1, corpus.docs[m1], corpus.tfs[m1]), N.SS_ESTATE),
            ("a tier of whole lists", lambda sh: (sh.upload_lexical_fields(3000, sdl, BOOST, *sdense),
                                                  sh.append_sparse_fields(*srare[:4], positions=srare[4])), N.SS_ESTATE),
            ("an image without merged lists", lambda sh: sh.commit_level_fields(0, sdl, far, *sdense[:4]), N.SS_ENOTSUP)):
        sh = S.Shard(0)
        try:
            build(sh)
            if want == N.SS_ENOTSUP:
                assert sh.fields_info()[:2] == (3, False), "the boosts are not far enough apart"
            with_pos = want != N.SS_ENOTSUP
            ask = lambda: _answer(N, sh, sh.make_queries([[0, 1], [2]], S.QueryType.Intersection, field_filter=None if with_pos else [0]), 10,
                                  S.ResultType.TopkCount)  # (an image without merged lists answers filtered queries only)
            before = (sh.sparse_info(), ask())
            assert not _refused(before[1]) and int(before[1][3][1]) > 0, what
            assert code_of(lambda: sh.commit_sparse_level_fields(0, *srare[:4], positions=srare[4] if with_pos else None)) == want, what
            after = (sh.sparse_info(), ask())
            assert before[0] == after[0], what
            _same_result(before[1], after[1], what)
        finally:
            sh.close()


def _dense_terms(c, lo, hi, n_terms):
    """the level's entries of the first n_terms terms as ONE dense call's arrays (with positions)"""
    _, lo_, ld, lf, lt, lp = c.level(lo, hi, n_terms)
    return lo_, ld, lf, lt, lp


def _shrunk(c, lo, hi):
    ldl, lo_, ld, lf, lt, lp = c.level(lo, hi, ND)
    return ldl, BOOST, lo_, ld, lf, lt, lp


HOST_LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "seekstorm_amd", "lib", "libseekstorm_host.so")


def test_cpp_mirror_commits_a_tiered_level(S, N, corpus):
    """Shard::commit_level_fields of the C++ mirror (ssh_commit_level_fields: one CSR of all known terms, n_dense_terms) for two levels,
    against the Python shard's answers after the same steps"""
    from test_host_cpp import _cpp_lexical_ex, P, u8p, u16p, u32p, u64p, f32p
    N.lib()
    if not os.path.exists(HOST_LIB):
        from seekstorm_amd import build as B
        B.build_host()
    H = C.CDLL(HOST_LIB)
    H.ssh_index_create.restype = C.c_void_p
    H.ssh_index_create.argtypes = [C.c_int, C.POINTER(C.c_int)]
    H.ssh_index_destroy.argtypes = [C.c_void_p]
    H.ssh_commit_level_fields.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, u8p, f32p, C.c_uint32, C.c_uint32, u64p, u32p, u8p,
                                          u16p, u16p, C.c_uint64]
    H.ssh_search_lexical_shard_ex.argtypes = [C.c_void_p, C.c_int, u32p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                              C.c_uint32, C.c_void_p, u32p, C.c_uint32, C.POINTER(C.c_uint16), C.c_uint32, C.c_void_p,
                                              C.c_uint32, C.c_uint32, u64p, f32p, u64p]
    boost = np.asarray(BOOST, np.float32)
    ix = H.ssh_index_create(1, None)
    psh = S.Shard(0)
    try:
        for step in ((0, 0, LVL, 9), (1, LVL, LVL + 3000, 9)):
            lv, lo, hi, nt = step
            ldl, lo_, ld, lf, lt, lp = corpus.level(lo, hi, nt)
            assert H.ssh_commit_level_fields(ix, 0, lv, hi - lo, 3, P(np.ascontiguousarray(ldl.reshape(-1)), u8p), P(boost, f32p), nt, ND, P(lo_, u64p),
                                             P(ld, u32p), P(lf, u8p), P(lt, u16p), P(lp, u16p), len(lp)) == 0, step
            _commit(psh, corpus, step, True)
        for terms, neg in (([0, 1], []), ([6, 0], []), ([8], []), ([7, 2], [1]), ([6, 7, 8], []), ([1, 2], [6])):
            for qt in (S.QueryType.Union, S.QueryType.Intersection):
                ro = psh.search_lexical_shard(terms, qt, 0, 10, S.ResultType.TopkCount, strict=True, not_terms=neg)
                cd, cs, ctot = _cpp_lexical_ex(H, ix, terms, int(qt), 0, 10, 2, not_terms=neg)
                assert ctot == ro.result_count_total, (terms, neg, qt)
                assert np.allclose(cs, np.array([r.score for r in ro.results], np.float32), rtol=1e-6), (terms, neg, qt)
                assert list(cd) == [r.doc_id for r in ro.results], (terms, neg, qt)
        assert psh.search_lexical_shard([6, 0], S.QueryType.Union, 0, 10, S.ResultType.TopkCount, strict=True).result_count_total > 0
    finally:
        H.ssh_index_destroy(ix)
        psh.close()
