"""ss_bm25_commit_level_fields: levels of an image with several indexed fields kept in HBM, the image -- per-field lists, merged lists,
probe rows, field-tagged positions -- rebuilt on the device after every commit, built aside and swapped in at once.  After every step
the shard must answer exactly (np.array_equal) like a fresh shard that got ONE ss_bm25_upload_fields[_positions] of the same prefix.
A level is 65 536 docs and a sub-block 4096, so the corpus is two full levels and a partial third, with small dfs."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LVL = 65536
N_DOCS = 2 * LVL + 30_000
PARTIAL = 12_000          # docs of level 2 when it is first committed
BOOST = [2.0, 1.0, 0.5]
#        0      1      2      3      4      5    6    7   8 (nobody's)  9 (known from the last step on)
DFS = [9_000, 6_000, 12_000, 3_000, 4_000, 400, 900, 60, 0, 200]
EMPTY, LATE = 8, 9
ABSENT_L1, ONE_FIELD = 5, 6   # a term without a posting in level 1; a term that lives in field 1 only
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


class Corpus:
    def __init__(self, dl, offs, docs, fields, tfs, positions):
        self.dl, self.offs, self.docs, self.fields, self.tfs, self.positions = dl, offs, docs, fields, tfs, positions
        self.eterm = np.repeat(np.arange(len(offs) - 1), np.diff(offs.astype(np.int64)))
        self.pterm_mask_src = np.repeat(np.arange(len(docs)), tfs.astype(np.int64))  # entry of every position

    def cut(self, lo, hi, n_terms, col0):
        """entries with lo <= doc < hi of the first n_terms terms, and the length bytes of docs [col0, hi)"""
        m = (self.docs >= lo) & (self.docs < hi) & (self.eterm < n_terms)
        offs = np.zeros(n_terms + 1, np.uint64)
        offs[1:] = np.cumsum(np.bincount(self.eterm[m], minlength=n_terms)[:n_terms])
        return (np.ascontiguousarray(self.dl[:, col0:hi]), offs, self.docs[m], self.fields[m], self.tfs[m],
                np.ascontiguousarray(self.positions[m[self.pterm_mask_src]]))

    def level(self, lo, hi, n_terms):
        return self.cut(lo, hi, n_terms, lo)

    def prefix(self, hi, n_terms):
        return self.cut(0, hi, n_terms, 0)


def _edit(offs, docs, fields, tfs, positions, edit):
    """the CSR as {term: {(doc, field): [positions]}}, edited, and back"""
    pstart = np.concatenate([[0], np.cumsum(tfs.astype(np.int64))])
    terms = []
    for t in range(len(offs) - 1):
        terms.append({(int(docs[j]), int(fields[j])): positions[pstart[j]:pstart[j + 1]].tolist() for j in range(int(offs[t]), int(offs[t + 1]))})
    edit(terms)
    o, d, f, tf, ps = [0], [], [], [], []
    for e in terms:
        for (dd, ff) in sorted(e):
            d.append(dd); f.append(ff); tf.append(len(e[(dd, ff)])); ps += sorted(e[(dd, ff)])
        o.append(len(d))
    return np.asarray(o, np.uint64), np.asarray(d, np.uint32), np.asarray(f, np.uint8), np.asarray(tf, np.uint16), np.asarray(ps, np.uint16)


@pytest.fixture(scope="module")
def corpus(O):
    from test_gpu_phrase import _corpus_fields
    plant = [([0, 1], 0, 300), ([0, 1], 2, 200), ([0, 1, 2], 1, 150), ([2, 0, 2], 0, 100), ([3, 4], 2, 60), ([1, 1], 2, 80), ([4, 0, 1], 0, 70)]
    cross = [(0, 1, 500), (3, 4, 300)]
    dl, offs, docs, fields, tfs, positions = _corpus_fields(O, N_DOCS, 3, DFS, 23, plant, cross)

    def edit(terms):
        terms[ABSENT_L1] = {k: v for k, v in terms[ABSENT_L1].items() if not LVL <= k[0] < 2 * LVL}
        terms[ONE_FIELD] = {k: v for k, v in terms[ONE_FIELD].items() if k[1] == 1}
        terms[LATE] = {k: v for k, v in terms[LATE].items() if k[0] >= 2 * LVL + PARTIAL}  # (only the re-committed level has seen it)
        for i, d in enumerate(EDGE_DOCS):  # postings on the first and the last doc of a sub-block and of a level
            terms[0].setdefault((d, i % 3), [7])
            terms[7].setdefault((d, 1), [3, 9])
        terms[7][(4096, 0)] = [1]; terms[7][(4096, 2)] = [2, 5, 8]  # ... and one doc with the term in all three fields

    offs, docs, fields, tfs, positions = _edit(offs, docs, fields, tfs, positions, edit)
    c = Corpus(dl, offs, docs, fields, tfs, positions)
    # what the corpus must hold, so that nothing below passes vacuously
    of = lambda t: slice(int(offs[t]), int(offs[t + 1]))
    assert not np.any((docs[of(ABSENT_L1)] >= LVL) & (docs[of(ABSENT_L1)] < 2 * LVL)) and np.any(docs[of(ABSENT_L1)] < LVL)
    assert set(fields[of(ONE_FIELD)].tolist()) == {1} and len(docs[of(ONE_FIELD)]) > 100
    assert any(np.sum(docs[of(t)] == d) == 3 for t in (0, 7) for d in (4096,))
    assert offs[EMPTY] == offs[EMPTY + 1] and offs[LATE + 1] - offs[LATE] >= 1 and docs[of(LATE)].min() >= 2 * LVL + PARTIAL
    for d in EDGE_DOCS:
        assert d in docs[of(0)] and d in docs[of(7)]
    seg = np.bincount((c.eterm * 3 + fields).astype(np.int64) * 64 + (docs >> 12))  # (term, field, sub-block) segment lengths
    assert np.any((seg > 0) & (seg % 4 == 0)) and np.any(seg % 4 != 0)
    return c


SETS = [[0, 1], [1, 2, 3], [4], [0, 2, 3, 4], [2, 3], [5, 0], [1, 5, 4], [7, 0], [6, 2], [8, 0], [9, 1], [7]]
NOTS = [[], [4], [], [], [0], [], [2], [], [1], [], [], [6]]
PHRASES = [[0, 1], [1, 0], [0, 1, 2], [2, 0, 2], [3, 4], [1, 1], [4, 0, 1], [7, 0], [6, 6]]


def _answer(N, sh, q, k, rt):
    try:
        return tuple(np.copy(x) for x in sh.search_lexical_batch(q, k, rt, reference_shortcuts=False))
    except N.SeekStormHipError as e:
        return ("refused", e.code)


def _refused(a):
    return isinstance(a[0], str)


def _same_result(a, b, what):
    assert len(a) == len(b) and type(a[0]) is type(b[0]), (what, a[:2], b[:2])
    for x, y in zip(a, b):
        assert np.array_equal(x, y), what


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


def _compare(S, N, inc, one, nt, positions, what, must_answer=True):
    assert inc.fields_info() == one.fields_info(), what
    terms = np.arange(nt, dtype=np.uint32)
    assert np.array_equal(inc.posting_count(terms), one.posting_count(terms)), what
    for (name, qi), (_, qo) in zip(_queries(S, inc, nt, positions), _queries(S, one, nt, positions)):
        assert np.array_equal(qi.view(np.uint8), qo.view(np.uint8)), ("idf differs: the two images disagree on N or df", what, name)
    a, b = _all_answers(S, N, inc, nt, positions), _all_answers(S, N, one, nt, positions)
    for key in a:
        _same_result(a[key], b[key], (what, key))
        if must_answer:
            assert not _refused(a[key]), (what, key, a[key])
    return a


def _oracle(S, O, c, sh, hi, nt, positions):
    pdl, po, pd, pf, pt, pp = c.prefix(hi, nt)
    for terms, qt, op in (([0, 1], S.QueryType.Union, O.OP_OR), ([1, 2, 3], S.QueryType.Intersection, O.OP_AND)):
        d, s, cnt, tot = sh.search_lexical_batch(sh.make_queries([terms], qt), 10, reference_shortcuts=False)
        od, os_, otot, _ = O.search_fields_exhaustive(hi, pdl, BOOST, po, pd, pf, pt, terms, op, 10)
        assert int(tot[0]) == otot and int(cnt[0]) == len(od) and np.allclose(s[0][:len(od)], os_, rtol=1e-4), (hi, terms)
    if positions:
        d, s, cnt, tot = sh.search_lexical_batch(sh.make_queries([[0, 1]], S.QueryType.Phrase), 10)
        od, os_, otot = O.search_fields_phrase(hi, pdl, BOOST, po, pd, pf, pt, pp, [0, 1], [0, 1], 10, reference_loop=False)
        assert otot >= 100 and int(tot[0]) == otot and int(cnt[0]) == len(od) and np.allclose(s[0][:len(od)], os_, rtol=1e-4), hi


def _commit(sh, c, step, positions, boost=BOOST):
    lv, lo, hi, nt = step
    ldl, lo_, ld, lf, lt, lp = c.level(lo, hi, nt)
    sh.commit_level_fields(lv, ldl, boost, lo_, ld, lf, lt, positions=lp if positions else None)


def _upload(one, c, step, positions, boost=BOOST):
    _, _, hi, nt = step
    pdl, po, pd, pf, pt, pp = c.prefix(hi, nt)
    one.upload_lexical_fields(hi, pdl, boost, po, pd, pf, pt, pp if positions else None)


def test_committed_levels_equal_one_upload_with_positions(S, N, O, corpus):
    """levels 0 and 1, a partial level 2, level 2 re-committed whole with a term no level had seen: after every step the same
    fields_info, posting counts, query records (idf), and bit-equal answers -- unions, intersections, field filters, NOT terms,
    phrases with and without a field filter, k 10 and 100, TopkCount and Count -- as one upload of the prefix; three queries against the oracle"""
    inc, one = S.Shard(0), S.Shard(0)
    try:
        for step in STEPS:
            _commit(inc, corpus, step, True)
            _upload(one, corpus, step, True)
            assert inc.fields_info() == (3, True, True)
            _compare(S, N, inc, one, step[3], True, step)
            _oracle(S, O, corpus, inc, step[2], step[3], True)
            nl, nbytes = inc.incremental_info()[:2]
            assert nl == step[0] + 1 and nbytes > 0
        # a term nobody holds, and the late term: known, with the dfs of the one-shot image
        assert int(inc.posting_count(np.array([EMPTY], np.uint32))[0]) == 0 and int(inc.posting_count(np.array([LATE], np.uint32))[0]) >= 1
        # the cross-field neighbours are no phrase
        t_ph = int(inc.search_lexical_batch(inc.make_queries([[3, 4]], S.QueryType.Phrase), 10)[3][0])
        t_and = int(inc.search_lexical_batch(inc.make_queries([[3, 4]], S.QueryType.Intersection), 10, reference_shortcuts=False)[3][0])
        assert 60 <= t_ph < t_and - 250
    finally:
        inc.close(); one.close()


def test_committed_levels_without_positions(S, N, O, corpus):
    """the same steps with positions=None equal ss_bm25_upload_fields; a phrase then raises; levels with and without positions do not mix"""
    inc, one = S.Shard(0), S.Shard(0)
    try:
        for step in STEPS:
            _commit(inc, corpus, step, False)
            _upload(one, corpus, step, False)
            assert inc.fields_info() == (3, True, False)
            _compare(S, N, inc, one, step[3], False, step)
        _oracle(S, O, corpus, inc, N_DOCS, 10, False)
        with pytest.raises(N.SeekStormHipError):
            inc.search_lexical_batch(inc.make_queries([[0, 1]], S.QueryType.Phrase), 10)
        before = _all_answers(S, N, inc, 10, False)
        with pytest.raises(N.SeekStormHipError) as e:
            _commit(inc, corpus, STEPS[3], True)  # positions on an image whose levels have none
        assert e.value.code == N.SS_EINVAL
        after = _all_answers(S, N, inc, 10, False)
        for key in before:
            _same_result(before[key], after[key], key)
    finally:
        inc.close(); one.close()
    inc = S.Shard(0)
    try:
        _commit(inc, corpus, STEPS[0], True)
        with pytest.raises(N.SeekStormHipError) as e:
            _commit(inc, corpus, STEPS[1], False)  # ... and the other way round
        assert e.value.code == N.SS_EINVAL and inc.incremental_info()[0] == 1
    finally:
        inc.close()


def test_boosts_too_far_apart_for_merged_lists(S, N, corpus):
    """boosts whose merged weights span more than the weight code: the one-shot upload builds no merged lists, and so do the commits;
    without positions they equal that upload (refusing the same queries), with positions the commit is refused (SS_ENOTSUP)"""
    boost = [1.0e6, 1.0, 1.0e-6]
    inc, one = S.Shard(0), S.Shard(0)
    try:
        for step in STEPS:
            _commit(inc, corpus, step, False, boost)
            _upload(one, corpus, step, False, boost)
            assert one.fields_info() == (3, False, False), "the upload built merged lists: the boosts are not far enough apart"
            _compare(S, N, inc, one, step[3], False, step, must_answer=False)
        a = _answer(N, inc, inc.make_queries([[0, 1]], S.QueryType.Intersection, field_filter=[1]), 10, S.ResultType.TopkCount)
        assert not _refused(a) and int(a[3][0]) > 0  # (something IS answered on such an image)
    finally:
        inc.close(); one.close()
    inc = S.Shard(0)
    try:
        with pytest.raises(N.SeekStormHipError) as e:
            _commit(inc, corpus, STEPS[0], True, boost)
        assert e.value.code == N.SS_ENOTSUP
        with pytest.raises(N.SeekStormHipError) as e:
            _upload(inc, corpus, STEPS[0], True, boost)  # (the upload refuses the same)
        assert e.value.code == N.SS_ENOTSUP
    finally:
        inc.close()


def _b4(b):
    """SmallFloat byte4_to_int"""
    b = int(b)
    if b < 24:
        return b
    i = b - 24
    bits, shift = i & 7, i >> 3
    return 24 + bits if shift == 0 else 24 + ((bits | 8) << (shift - 1))


def _uncodable_entry(offs, docs, fields, tfs):
    """a field-1 entry with tf 1 of a doc that holds every one of its field-1 terms in field 0 as well"""
    et = np.repeat(np.arange(len(offs) - 1), np.diff(offs.astype(np.int64)))
    key = et.astype(np.int64) << 32 | docs.astype(np.int64)  # (term, doc)
    paired = np.isin(key, key[fields == 0])
    lone = np.unique(docs[(fields == 1) & ~paired])          # docs with a field-1 term that field 0 lacks
    cand = np.flatnonzero((fields == 1) & (tfs == 1) & paired & ~np.isin(docs, lone))
    assert len(cand)
    return int(cand[0])


def test_a_refused_commit_changes_nothing(S, N, corpus):
    """after two good levels a third is refused three ways -- a weight the code cannot hold, a wrong n_positions, an entry out of
    (doc, field) order --: the answers stay bit-identical, two levels stay, and the correct third level then commits and matches"""
    inc, one = S.Shard(0), S.Shard(0)
    try:
        _commit(inc, corpus, STEPS[0], True)
        _commit(inc, corpus, STEPS[1], True)
        nt = STEPS[1][3]
        before = _all_answers(S, N, inc, nt, True)
        lv, lo, hi, _ = STEPS[3]
        ldl, lo_, ld, lf, lt, lp = corpus.level(lo, hi, 10)

        def refused(code, *args, **kw):
            with pytest.raises(N.SeekStormHipError) as e:
                inc.commit_level_fields(lv, *args, **kw)
            assert e.value.code == code, e.value
            after = _all_answers(S, N, inc, nt, True)
            for key in before:
                _same_result(before[key], after[key], key)
                assert not _refused(before[key])
            assert inc.incremental_info()[0] == 2

        # (a) a field-1 entry with tf 1 whose doc gets SmallFloat's largest length in field 1: its weight lies below 2^-14.  Every
        # term the doc holds in field 1 it holds in field 0 too, so every MERGED weight of the doc stays in range, the image keeps its
        # merged lists, and the refusal is the fill kernel's count of uncodable weights (of the field-1 list)
        j = _uncodable_entry(lo_, ld, lf, lt)
        bad_dl = ldl.copy()
        bad_dl[1, int(ld[j]) - lo] = 255
        table = np.array([_b4(b) for b in range(256)], np.float64)
        psum = table[corpus.dl[:, :lo]].sum() + table[bad_dl].sum()
        comp = np.float32(1.2) * (np.float32(0.25) + np.float32(0.75) * np.float32(_b4(255)) / np.float32(psum / hi))
        assert 2.2 / (1.0 + float(comp)) < 2.0 ** -14 / 2
        refused(N.SS_ENOTSUP, bad_dl, BOOST, lo_, ld, lf, lt, positions=lp)
        # ... and on levels without positions, where nothing but that count can refuse the level
        nop = S.Shard(0)
        try:
            _commit(nop, corpus, STEPS[0], False)
            _commit(nop, corpus, STEPS[1], False)
            with pytest.raises(N.SeekStormHipError) as e:
                nop.commit_level_fields(lv, bad_dl, BOOST, lo_, ld, lf, lt)
            assert e.value.code == N.SS_ENOTSUP and nop.incremental_info()[0] == 2
        finally:
            nop.close()
        # (b) one position too few
        refused(N.SS_EINVAL, ldl, BOOST, lo_, ld, lf, lt, positions=lp[:-1])
        # (c) two entries of a term swapped
        a = int(lo_[2])
        sd, sf, st = ld.copy(), lf.copy(), lt.copy()
        assert lo_[3] - lo_[2] >= 2
        sd[[a, a + 1]] = ld[[a + 1, a]]; sf[[a, a + 1]] = lf[[a + 1, a]]
        if lt[a] != lt[a + 1]:  # keep sum(tf) = n_positions, so that only the ORDER is wrong
            st[[a, a + 1]] = lt[[a + 1, a]]
        refused(N.SS_EINVAL, ldl, BOOST, lo_, sd, sf, st, positions=lp)
        # the correct level
        inc.commit_level_fields(lv, ldl, BOOST, lo_, ld, lf, lt, positions=lp)
        _upload(one, corpus, STEPS[3], True)
        _compare(S, N, inc, one, 10, True, "after the refusals")
        assert inc.incremental_info()[0] == 3
    finally:
        inc.close(); one.close()


def test_entry_codes(S, N, corpus):
    """level gap, a partial level that is not the last, a changed field count, a shrinking vocabulary: SS_EINVAL; an image built another
    way, either direction: SS_ESTATE; a sparse tier: SS_ENOTSUP -- and the image goes on serving every time"""
    small = (0, 0, 3000, 9)
    ldl, lo_, ld, lf, lt, lp = corpus.level(0, 3000, 9)
    q_of = lambda sh, **kw: sh.make_queries([[0, 1], [2]], S.QueryType.Union, **kw)
    m1 = (corpus.fields == 0) & (corpus.docs < 3000) & (corpus.eterm < 9)  # field 0 of the same docs as a ONE-field level
    o1 = np.zeros(10, np.uint64); o1[1:] = np.cumsum(np.bincount(corpus.eterm[m1], minlength=9)[:9])
    one_field_level = (corpus.dl[0, :3000], o1, corpus.docs[m1], corpus.tfs[m1])

    def serving(sh, before):
        _same_result(_answer(N, sh, q_of(sh), 10, S.ResultType.TopkCount), before, "still serving")

    def code_of(call):
        with pytest.raises(N.SeekStormHipError) as e:
            call()
        return e.value.code

    inc = S.Shard(0)
    try:
        _commit(inc, corpus, small, True)
        before = _answer(N, inc, q_of(inc), 10, S.ResultType.TopkCount)
        assert not _refused(before) and int(before[3][0]) > 0
        l1 = corpus.level(LVL, LVL + 3000, 9)
        assert code_of(lambda: inc.commit_level_fields(5, l1[0], BOOST, *l1[1:5], positions=l1[5])) == N.SS_EINVAL   # a gap
        assert code_of(lambda: inc.commit_level_fields(1, l1[0], BOOST, *l1[1:5], positions=l1[5])) == N.SS_EINVAL   # level 0 is partial
        m = lf < 2
        o2 = np.zeros(10, np.uint64); o2[1:] = np.cumsum(np.bincount(np.repeat(np.arange(9), np.diff(lo_.astype(np.int64)))[m], minlength=9))
        assert code_of(lambda: inc.commit_level_fields(0, ldl[:2], BOOST[:2], o2, ld[m], lf[m], lt[m])) == N.SS_EINVAL  # two fields now
        serving(inc, before)
        assert code_of(lambda: inc.append_level_fields(0, ldl, BOOST, lo_, ld, lf, lt)) == N.SS_ESTATE              # the old entry on these levels
        assert code_of(lambda: inc.append_level(0, *one_field_level)) == N.SS_ESTATE                                 # the one-field entry
        serving(inc, before)
        assert inc.incremental_info()[0] == 1
    finally:
        inc.close()
    # a shrinking vocabulary: a second level that knows fewer terms
    inc = S.Shard(0)
    try:
        _commit(inc, corpus, STEPS[0], False)
        before = _answer(N, inc, q_of(inc), 10, S.ResultType.TopkCount)
        l1 = corpus.level(LVL, LVL + 3000, 8)
        assert code_of(lambda: inc.commit_level_fields(1, l1[0], BOOST, *l1[1:5])) == N.SS_EINVAL
        serving(inc, before)
    finally:
        inc.close()
    # images built another way: a one-shot upload, one-field levels, levels of the host-kept entry; a sparse tier
    pdl, po, pd, pf, pt, pp = corpus.prefix(20_000, 8)
    cut = int(po[5])  # terms 0..4 dense, 5..7 the sparse tier
    assert np.all(np.diff(po.astype(np.int64))[5:] > 0)
    for build, want in ((lambda sh: sh.upload_lexical_fields(20_000, pdl, BOOST, po, pd, pf, pt, pp), N.SS_ESTATE),
                        (lambda sh: sh.append_level_fields(0, ldl, BOOST, lo_, ld, lf, lt), N.SS_ESTATE),
                        (lambda sh: (sh.upload_lexical_fields(20_000, pdl, BOOST, po[:6], pd[:cut], pf[:cut], pt[:cut]),
                                     sh.append_sparse_fields(po[5:] - po[5], pd[cut:], pf[cut:], pt[cut:])), N.SS_ENOTSUP)):
        sh = S.Shard(0)
        try:
            build(sh)
            before = _answer(N, sh, q_of(sh), 10, S.ResultType.TopkCount)
            assert not _refused(before)
            assert code_of(lambda: sh.commit_level_fields(0, ldl, BOOST, lo_, ld, lf, lt, positions=lp)) == want
            serving(sh, before)
        finally:
            sh.close()
    sh = S.Shard(0)
    try:
        sh.append_level(0, *one_field_level)
        assert code_of(lambda: sh.commit_level_fields(0, ldl, BOOST, lo_, ld, lf, lt, positions=lp)) == N.SS_ESTATE
        assert sh.incremental_info()[0] == 1
    finally:
        sh.close()
