"""ss_bm25_delete_by_query: the docs a lexical search selects become tombstones in one call (-m gpu).

The pattern of test_gpu_add_deleted.py: shard `one` gets the call, shard `two` gets set_deleted(old set | expected), and a flat list of
answers -- lexical unions and intersections, a filtered search and a facet count, a vector search with observed counts, the empty query
in both directions -- must be equal on both; search_docs(n_docs, doc_ascending=True) must list exactly the docs alive in numpy.  Every
output is an integer or a stored bit pattern, so every comparison is ==.

The expected sets come from numpy over the corpus arrays, never from the library: set algebra over posting arrays, NOT lists, facet
values and positions.  n_docs = 20 035: 627 tombstone words, an odd number, so the image's last u64 group is half outside the
bitmap; no multiple of 64 or 4096.  Term 4's three docs include the last doc.  Besides the five terms of df 0.6 / 0.25 / 0.05 / 0.01 /
3 docs the world holds a sixth of df 0.55: an intersection is ranked under all_terms_frequent only when EVERY term occurs in half of the
docs (the library checks the posting counts again and ignores the bit otherwise), which takes two frequent terms.

Prior tombstone states of the whole-set cases: no bitmap at all; a two-word bitmap (ids <= 63), which the call must grow; a bitmap
longer than the image (one id beyond n_docs).  In the two states that have a bitmap some matching docs are already deleted (asserted);
the state without a bitmap has, by its nature, none."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_DOCS, DIM = 20_035, 64
DF = [0.6, 0.25, 0.05, 0.01]
RARE = [5, 9_000, N_DOCS - 1]          # term 4
EVERY = [5, 40]                        # docs that hold every dense term and the phrase (1, 2): matching docs below id 64
OFF_CAT, OFF_PERM = 0, 4               # the facet record: an i32 of few values, a u32 permutation of range(n_docs)
CAT_LO, CAT_HI = 2, 5
STATES = {"no_bitmap": [], "two_words": [0, 1, 5, 31, 32, 40, 47, 63], "longer": [3, 5, 40, 64, 4095, 4096, 12_345, N_DOCS + 70]}
SS_EINVAL, SS_ENOTSUP, SS_ESTATE = -1, -4, -5
ALL = 0xFFFFFFFFFFFFFFFF


@pytest.fixture(scope="module")
def S():
    import seekstorm_amd
    return seekstorm_amd


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


def _postings(rng, n_docs, doc_lists, plant=()):
    """doc lists -> CSR arrays with positions (tf = min(geometric, 30) distinct positions below 60); plant = [(term a, term b, docs)]:
    a at p and b at p + 1 written into the docs.  -> (offs, docs, tfs, positions, pos_of): pos_of[t] = {doc: set of positions}"""
    pos_of = []
    for ds in doc_lists:
        pos_of.append({int(d): set(int(x) for x in rng.choice(60, int(min(rng.geometric(0.12), 30)), replace=False)) for d in ds})
    for a, b, ds in plant:
        for d in ds:
            st = int(rng.integers(0, 59))
            pos_of[a].setdefault(int(d), set()).add(st)
            pos_of[b].setdefault(int(d), set()).add(st + 1)
    offs, docs, tfs, positions = [0], [], [], []
    for po in pos_of:
        for d in sorted(po):
            ps = sorted(po[d])
            docs.append(d); tfs.append(len(ps)); positions += ps
        offs.append(len(docs))
    return np.asarray(offs, np.uint64), np.asarray(docs, np.uint32), np.asarray(tfs, np.uint16), np.asarray(positions, np.uint16), pos_of


class World:
    """the corpus arrays and numpy's view of them: has[t] = the docs of term t as a mask, tf[t] = its tfs by doc"""

    def __init__(self, O, seed=11):
        rng = np.random.default_rng(seed)
        lists = [np.union1d(rng.choice(N_DOCS, int(df * N_DOCS), replace=False), EVERY) for df in DF] + [np.array(RARE)]
        # term 5, a second FREQUENT term (df 0.55): the library honours all_terms_frequent only where every term is in half of the docs
        lists.append(np.union1d(np.random.default_rng(seed + 1).choice(N_DOCS, int(0.55 * N_DOCS), replace=False), EVERY))
        planted = np.union1d(rng.choice(N_DOCS, 300, replace=False), EVERY)
        self.dl = O.lex_doclen(N_DOCS)
        self.offs, self.docs, self.tfs, self.positions, self.pos_of = _postings(rng, N_DOCS, lists, [(1, 2, planted)])
        self.n_terms = len(lists)
        self.has = np.zeros((self.n_terms, N_DOCS), bool)
        self.tf = np.zeros((self.n_terms, N_DOCS), np.int64)
        for t in range(self.n_terms):
            a, b = int(self.offs[t]), int(self.offs[t + 1])
            self.has[t, self.docs[a:b]] = True
            self.tf[t, self.docs[a:b]] = self.tfs[a:b]
        self.cat = rng.integers(0, 7, N_DOCS).astype(np.int32)
        self.perm = rng.permutation(N_DOCS).astype(np.uint32)
        rec = np.zeros(N_DOCS, np.dtype([("cat", "<i4"), ("perm", "<u4")]))
        rec["cat"], rec["perm"] = self.cat, self.perm
        self.records = rec.view(np.uint8).reshape(N_DOCS, 8)
        self.rows = O.vec_gen(O.VEC_SEED, 0, N_DOCS, DIM)
        self.vq = O.vec_gen(O.VECQ_SEED, 0, 4, DIM)

    def term_postings(self, t):
        a, b = int(self.offs[t]), int(self.offs[t + 1])
        return self.docs[a:b], self.tfs[a:b]

    def phrase(self, a, b):
        m = np.zeros(N_DOCS, bool)
        pb = self.pos_of[b]
        for d, ps in self.pos_of[a].items():
            if d in pb and any(p + 1 in pb[d] for p in ps):
                m[d] = True
        return m

    def match(self, shape):
        """shape = (kind, terms, NOT terms, filtered) -> the docs that match, tombstones aside"""
        kind, terms, nots, filtered = shape
        if kind == "phrase":
            m = self.phrase(*terms)
        elif kind == "and":
            m = np.logical_and.reduce([self.has[t] for t in terms])
        else:
            m = np.logical_or.reduce([self.has[t] for t in terms])
        for t in nots:
            m = m & ~self.has[t]
        if filtered:
            m = m & (self.cat >= CAT_LO) & (self.cat < CAT_HI)
        return m

    def shard(self, S):
        sh = S.Shard(0)
        sh.upload_lexical(N_DOCS, self.dl, self.offs, self.docs, self.tfs, self.positions)
        sh.upload_facets(self.records)
        sh.upload_vectors(self.rows)
        return sh

    def queries(self, S, sh, shapes):
        qt = {"or": S.QueryType.Union, "and": S.QueryType.Intersection, "phrase": S.QueryType.Phrase}
        return sh.make_queries([list(s[1]) for s in shapes], [qt[s[0]] for s in shapes], [list(s[2]) for s in shapes])


FILTER = [(OFF_CAT, "i32", CAT_LO, CAT_HI)]
SHAPES = {"single": ("or", (1,), (), False), "union3": ("or", (1, 2, 4), (), False), "and2": ("and", (0, 1), (), False),
          "not": ("or", (0,), (2,), False), "filtered": ("or", (0, 3), (), True), "phrase": ("phrase", (1, 2), (), False)}


@pytest.fixture(scope="module")
def W(O):
    return World(O)


@pytest.fixture(scope="module")
def pair(S, W):
    one, two = W.shard(S), W.shard(S)
    yield one, two
    one.close()
    two.close()


def _answers(S, sh, W):
    """everything a tombstone can change, as a flat list of integer arrays"""
    out = []
    for terms, qt in (([[0, 1, 2], [1, 4]], S.QueryType.Union), ([[0, 1], [0, 1, 2]], S.QueryType.Intersection)):
        d, s, c, t = sh.search_lexical_batch(sh.make_queries(terms, qt), 100, S.ResultType.TopkCount)
        out += [d, s.view(np.uint32), c, t]
    q = sh.make_queries([[0, 3]], S.QueryType.Union)
    d, s, c, t = sh.search_lexical_batch(q, 50, S.ResultType.TopkCount, facet_filter=FILTER)
    out += [d, s.view(np.uint32), c, t]
    counts, outside, tot = sh.facet_count(q, OFF_CAT, "i32", range_lower_bounds=[0, 2, 4, 6])
    out += [counts, np.array([outside, tot])]
    d, s, c, t, ncl, obs = sh.search_vector_batch(W.vq, 50, with_observed=True)
    out += [d, s.view(np.uint32), c, t, np.asarray(ncl), np.asarray(obs)]
    for asc in (False, True):
        d, cnt, tot, _ = sh.search_docs(200, doc_ascending=asc)
        out += [d, np.array([cnt, tot])]
    return out


def _same(x, y):
    return len(x) == len(y) and all(np.array_equal(a, b) for a, b in zip(x, y))


def _alive(state, extra=()):
    a = np.ones(N_DOCS, bool)
    a[[d for d in state if d < N_DOCS]] = False
    a[np.asarray(extra, np.int64)] = False
    return a


def _check_pair(S, W, one, two, state, expected):
    """`one` after the call answers as `two` after set_deleted(state | expected), and lists exactly numpy's live docs"""
    two.set_deleted(sorted(set(state) | set(int(d) for d in expected)))
    assert _same(_answers(S, one, W), _answers(S, two, W))
    alive = _alive(state, expected)
    d, cnt, tot, _ = one.search_docs(N_DOCS, doc_ascending=True)
    assert tot == int(alive.sum()) and np.array_equal(d, np.nonzero(alive)[0])


def _raw(sh, q, n_sorts=0, sorts=None, offset=0, length=ALL, flags=0, doc_cap=N_DOCS, nq=None, handle=True, queries=True):
    """the entry itself -> (rc, matched, selected, deleted, docs buffer)"""
    from seekstorm_amd import _native as N
    nq = len(q) if nq is None else nq
    matched, selected = np.zeros(max(nq, 1), np.uint64), np.zeros(max(nq, 1), np.uint64)
    deleted = C.c_uint64(0)
    docs = np.full(max(doc_cap, 1), 0xFFFFFFFF, np.uint32)
    rc = N.lib().ss_bm25_delete_by_query(sh._h if handle else None, nq, q.ctypes.data_as(C.c_void_p) if queries else None, n_sorts,
                                         None if sorts is None else C.cast(sorts, C.c_void_p), offset, length, 0, None, flags,
                                         N.ptr(matched, N.u64p), N.ptr(selected, N.u64p), C.byref(deleted), N.ptr(docs, N.u32p), doc_cap)
    return rc, matched, selected, int(deleted.value), docs


# ---- 1. the whole match set, from three prior tombstone states
@pytest.mark.parametrize("state_name", list(STATES))
@pytest.mark.parametrize("shape_name", list(SHAPES))
def test_whole_match_set(S, W, pair, shape_name, state_name):
    one, two = pair
    shape, state = SHAPES[shape_name], STATES[state_name]
    m = W.match(shape)
    live = m & _alive(state)
    if state:
        assert (m & ~_alive(state)).any()  # some matching docs are deleted already
    one.set_deleted(state)
    q = W.queries(S, one, [shape])
    matched, selected, deleted, docs = one.delete_by_query(q, facet_filter=FILTER if shape[3] else None, return_docs=True)
    expected = np.nonzero(live)[0]
    assert int(matched[0]) == len(expected) and int(selected[0]) == len(expected) and deleted == len(expected)
    assert np.array_equal(docs, expected)
    _check_pair(S, W, one, two, state, expected)


# ---- 2. the call again, a dry run, a doc buffer one short
def test_repeat_dry_run_and_short_buffer(S, W, pair):
    one, two = pair
    state, shape = STATES["two_words"], SHAPES["union3"]
    expected = np.nonzero(W.match(shape) & _alive(state))[0]
    one.set_deleted(state)
    q = W.queries(S, one, [shape])
    before = _answers(S, one, W)
    rc, matched, _, deleted, _ = _raw(one, q, doc_cap=len(expected) - 1)
    assert rc == SS_EINVAL and deleted == len(expected)
    assert _same(_answers(S, one, W), before)
    dry = one.delete_by_query(q, dry_run=True, return_docs=True)
    assert _same(_answers(S, one, W), before)
    real = one.delete_by_query(q, return_docs=True)
    for a, b in zip(dry, real):
        assert np.array_equal(a, b)
    assert real[2] == len(expected) and np.array_equal(real[3], expected)
    _check_pair(S, W, one, two, state, expected)
    after = _answers(S, one, W)
    matched, selected, deleted, docs = one.delete_by_query(q, return_docs=True)
    assert int(matched[0]) == 0 and int(selected[0]) == 0 and deleted == 0 and len(docs) == 0
    assert _same(_answers(S, one, W), after)


# ---- 3. pages under the permutation column: numpy alone decides them
@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("page", ["first10", "across_pass", "beyond", "empty"])
def test_pages_under_a_sort(S, W, pair, page, descending):
    one, two = pair
    state, shape = STATES["two_words"], SHAPES["single"]
    live = np.nonzero(W.match(shape) & _alive(state))[0]
    n = len(live)
    assert n > 1100
    offset, length = {"first10": (0, 10), "across_pass": (7, 1030), "beyond": (n, 5), "empty": (3, 0)}[page]
    order = live[np.argsort(W.perm[live])]
    if descending:
        order = order[::-1]
    expected = np.sort(order[offset:offset + length])
    one.set_deleted(state)
    q = W.queries(S, one, [shape])
    matched, selected, deleted, docs = one.delete_by_query(q, offset, length, result_sort=[(OFF_PERM, "u32", descending)], return_docs=True)
    assert int(matched[0]) == n and int(selected[0]) == len(expected) and deleted == len(expected)
    assert np.array_equal(docs, expected)
    _check_pair(S, W, one, two, state, expected)


# ---- 4. one page by score
def _score_page(W, shape, state):
    """the first (offset, length) of a fixed list whose exact scores at both page edges differ by more than 1e-4 relative from their
    neighbours outside the page -> (offset, length, the page's docs); None if no candidate qualifies"""
    from oracle import naive
    ids, sc = naive.bm25_exact(N_DOCS, W.dl, [W.term_postings(t) for t in shape[1]], shape[0] == "and", deleted=[d for d in state if d < N_DOCS])
    order = np.lexsort((ids, -sc))
    ids, sc = ids[order], sc[order]
    for offset, length in ((5, 40), (11, 64), (3, 100), (20, 17), (64, 1000)):
        lo, hi = offset, offset + length
        if hi >= len(ids):
            continue
        if sc[lo - 1] - sc[lo] > 1e-4 * sc[lo - 1] and sc[hi - 1] - sc[hi] > 1e-4 * sc[hi - 1]:
            return offset, length, np.sort(ids[lo:hi]), len(ids)
    return None


def test_page_by_score(S, W, pair):
    one, two = pair
    state, shape = STATES["two_words"], ("or", (1, 2, 3), (), False)
    found = _score_page(W, shape, state)
    assert found is not None, "no candidate page with clear score edges"
    offset, length, expected, n = found
    one.set_deleted(state)
    q = W.queries(S, one, [shape])
    matched, selected, deleted, docs = one.delete_by_query(q, offset, length, return_docs=True)
    assert int(matched[0]) == n and int(selected[0]) == length and deleted == length
    assert np.array_equal(docs, expected)
    _check_pair(S, W, one, two, state, expected)


# ---- 5. batches: every page as of the call's begin, one union
def test_three_overlapping_queries(S, W, pair):
    one, two = pair
    state = STATES["longer"]
    shapes = [SHAPES["single"], ("or", (1, 2), (), False), SHAPES["and2"]]
    live = [W.match(s) & _alive(state) for s in shapes]
    one.set_deleted(state)
    matched, selected, deleted, docs = one.delete_by_query(W.queries(S, one, shapes), return_docs=True)
    assert [int(x) for x in matched] == [int(m.sum()) for m in live] and [int(x) for x in selected] == [int(m.sum()) for m in live]
    expected = np.nonzero(np.logical_or.reduce(live))[0]
    assert deleted == len(expected) and np.array_equal(docs, expected)
    _check_pair(S, W, one, two, state, expected)


def test_seventy_queries_two_chunks(S, W, pair):
    """the second chunk's queries match docs the first chunk deletes: a chunk built after an earlier one was committed would count less"""
    one, two = pair
    state = STATES["two_words"]
    first = [("or", (1 + i % 4,), (), False) for i in range(60)] + [("or", (0,), (), False)] * 4
    second = [("or", (0, 1), (), False), ("or", (1,), (), False), ("and", (0, 1), (), False), ("or", (2, 3), (), False), ("or", (4,), (), False),
              ("or", (0,), (2,), False)]
    shapes = first + second
    assert len(shapes) == 70
    live = [W.match(s) & _alive(state) for s in shapes]
    assert all((live[64 + i] & np.logical_or.reduce(live[:64])).any() for i in range(6))
    one.set_deleted(state)
    matched, selected, deleted, docs = one.delete_by_query(W.queries(S, one, shapes), return_docs=True)
    assert [int(x) for x in matched] == [int(m.sum()) for m in live]
    expected = np.nonzero(np.logical_or.reduce(live))[0]
    assert deleted == len(expected) and np.array_equal(docs, expected)
    _check_pair(S, W, one, two, state, expected)


# ---- 6. an intersection marked all_terms_frequent: its results are a subset of its matches
def test_all_terms_frequent_takes_the_page_path(S, W, pair):
    one, two = pair
    state, shape = STATES["two_words"], ("and", (0, 5), (), False)  # both terms in more than half of the docs
    live = W.match(shape) & _alive(state)
    ranked = live & (W.tf[0] >= 10) & (W.tf[5] >= 10)
    assert 0 < int(ranked.sum()) < int(live.sum())
    one.set_deleted(state)
    q = W.queries(S, one, [shape]).copy()
    q["op"][0] |= np.uint32(0x80000000)
    matched, selected, deleted, docs = one.delete_by_query(q, 0, int(live.sum()) + 7, return_docs=True)
    expected = np.nonzero(ranked)[0]
    assert int(matched[0]) == int(live.sum()) and int(selected[0]) == len(expected) and deleted == len(expected)
    assert np.array_equal(docs, expected)
    _check_pair(S, W, one, two, state, expected)


# ---- 7. refusals: each leaves the answers as they were
def test_refusals_change_nothing(S, W, pair):
    from seekstorm_amd import _native as N
    one, two = pair
    state = STATES["two_words"]
    one.set_deleted(state)
    two.set_deleted(state)
    want = _answers(S, two, W)
    q = W.queries(S, one, [SHAPES["single"]])
    assert _raw(one, q, handle=False)[0] == SS_EINVAL
    assert _raw(one, q, queries=False)[0] == SS_EINVAL
    assert _raw(one, q, flags=2)[0] == SS_EINVAL and _raw(one, q, flags=0x80000001)[0] == SS_EINVAL
    bad = q.copy()
    bad["term"][0, 0] = W.n_terms  # beyond the vocabulary
    assert _raw(one, bad)[0] == SS_EINVAL
    n, arr = one._result_sorts([(OFF_CAT, "string16", False)])  # a string sort field without a rank table
    assert _raw(one, q, n_sorts=n, sorts=arr)[0] == SS_ENOTSUP
    assert _same(_answers(S, one, W), want)
    bare = S.Shard(0)
    try:
        assert _raw(bare, q)[0] == SS_ESTATE
    finally:
        bare.close()
    # nothing to do is no refusal
    rc, matched, selected, deleted, _ = _raw(one, q, nq=0)
    assert rc == 0 and deleted == 0
    assert _same(_answers(S, one, W), want)
    assert N.lib().ss_bm25_delete_by_query(None, 0, None, 0, None, 0, 0, 0, None, 0, None, None, None, None, 0) == SS_EINVAL


# ---- World B: a dense vocabulary plus a sparse tier
def test_sparse_tier_whole_set_and_page(S, O):
    rng = np.random.default_rng(23)
    dense = [rng.choice(N_DOCS, int(df * N_DOCS), replace=False) for df in (0.5, 0.2, 0.04)]
    rare = [rng.choice(N_DOCS, n, replace=False) for n in (40, 15, 5)]
    offs, docs, tfs, positions, _ = _postings(rng, N_DOCS, dense)
    roffs, rdocs, rtfs, _, _ = _postings(rng, N_DOCS, rare)
    perm = rng.permutation(N_DOCS).astype(np.uint32)
    has = np.zeros((6, N_DOCS), bool)
    for t, ds in enumerate(dense + rare):
        has[t, ds] = True
    state = [0, 1, 63, 700] + [int(d) for d in rare[1][:3]]
    shards = []
    for _ in range(2):
        sh = S.Shard(0)
        sh.upload_lexical(N_DOCS, O.lex_doclen(N_DOCS), offs, docs, tfs)
        assert sh.append_sparse(roffs, rdocs, rtfs) == 3
        sh.upload_facets(perm.view(np.uint8).reshape(N_DOCS, 4))
        shards.append(sh)
    one, two = shards
    try:
        live = np.nonzero((has[2] | has[4]) & _alive(state))[0]  # a union naming a rare term
        for offset, length in ((0, None), (2, 20)):
            order = live[np.argsort(perm[live])]
            expected = live if length is None else np.sort(order[offset:offset + length])
            one.set_deleted(state)
            q = one.make_queries([[2, 4]], S.QueryType.Union)
            matched, selected, deleted, got = one.delete_by_query(q, offset, length, result_sort=None if length is None else [(0, "u32", False)],
                                                                  return_docs=True)
            assert int(matched[0]) == len(live) and int(selected[0]) == len(expected) and deleted == len(expected)
            assert np.array_equal(got, expected)
            two.set_deleted(sorted(set(state) | set(int(d) for d in expected)))
            alive = _alive(state, expected)
            for sh in (one, two):
                d, cnt, tot, _ = sh.search_docs(N_DOCS, doc_ascending=True)
                assert tot == int(alive.sum()) and np.array_equal(d, np.nonzero(alive)[0])
            qs = one.make_queries([[2, 4], [1, 3, 5]], S.QueryType.Union)
            a, b = one.search_lexical_batch(qs, 100), two.search_lexical_batch(qs, 100)
            assert all(np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y)
                       for x, y in zip(a, b))
    finally:
        one.close()
        two.close()


# ---- World C: three indexed fields
def test_three_fields_under_a_field_filter(S, O):
    rng = np.random.default_rng(31)
    n_fields, boost = 3, np.array([2.0, 1.0, 0.5], np.float32)
    dl = np.stack([O.lex_doclen(N_DOCS, seed=O.LEX_SEED + 7 * f) for f in range(n_fields)])
    offs, docs, fields, tfs = [0], [], [], []
    inside = np.zeros((3, n_fields, N_DOCS), bool)  # (term, field, doc) entries
    for t, df in enumerate((0.5, 0.3, 0.1)):
        for d in np.sort(rng.choice(N_DOCS, int(df * N_DOCS), replace=False)):
            for f in np.sort(rng.choice(n_fields, int(rng.integers(1, n_fields + 1)), replace=False)):
                docs.append(int(d)); fields.append(int(f)); tfs.append(int(min(rng.geometric(0.5), 12)))
                inside[t, f, d] = True
        offs.append(len(docs))
    arrays = (np.asarray(offs, np.uint64), np.asarray(docs, np.uint32), np.asarray(fields, np.uint8), np.asarray(tfs, np.uint16))
    state = [0, 2, 40, 63, 9_000]
    filt = (1,)
    passes = [inside[t, list(filt)].any(axis=0) for t in range(3)]  # the term occurs in a listed field
    shards = []
    for _ in range(2):
        sh = S.Shard(0)
        sh.upload_lexical_fields(N_DOCS, dl, boost, *arrays)
        shards.append(sh)
    one, two = shards
    try:
        for qt, m in ((S.QueryType.Intersection, passes[0] & passes[1]),   # the whole match set
                      (S.QueryType.Union, passes[0] | passes[2])):         # the match-set step refuses it: the page path answers
            live = np.nonzero(m & _alive(state))[0]
            terms = [0, 1] if qt == S.QueryType.Intersection else [0, 2]
            one.set_deleted(state)
            q = one.make_queries([terms], qt, field_filter=filt)
            matched, selected, deleted, got = one.delete_by_query(q, return_docs=True)
            assert int(matched[0]) == len(live) and int(selected[0]) == len(live) and deleted == len(live)
            assert np.array_equal(got, live)
            two.set_deleted(sorted(set(state) | set(int(d) for d in live)))
            qs = one.make_queries([[0, 1, 2], [1, 2]], S.QueryType.Union)
            a, b = one.search_lexical_batch(qs, 100), two.search_lexical_batch(qs, 100)
            assert all(np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y)
                       for x, y in zip(a, b))
            gone = set(state) | set(int(d) for d in live)
            assert int(a[3][0]) == int((inside[:3].any(axis=(0, 1)) & _alive(sorted(gone))).sum())
    finally:
        one.close()
        two.close()
