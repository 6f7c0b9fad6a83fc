"""Result sorts by String16 / String32 facets through rank tables kept on the device: ss_facet_set_string_ranks /
ss_facet_string_ranks, ss_bm25_search_sorted and ss_docs_search with string sort fields (-m gpu).

The expectation is a brute-force ordering by the strings' BYTES (Rust's String order) over the oracle's match set, written as
tests/test_gpu_parity.py::test_result_sort_by_a_string_facet writes it; docs and scores also equal, bit for bit, the host rank-column
path (Shard.string_facet_rank_column) on the same data.  Word list of that test: duplicates, the empty string, case pairs, multi-byte
UTF-8, a trailing space.  5 and 20 003 docs, tombstones at the edge docs."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

WORDS = ["zeta", "alpha", "Alpha", "beta", "éclair", "eclair", "omega", "beta", "a", "", "zz", "中文", "alpha ", "b", "B", "beta"]
REC = np.dtype([("s16", "<u2"), ("s32", "<u4"), ("h", "<u2"), ("f", "<f4"), ("u", "<u4")])
OFF = {n: REC.fields[n][1] for n in REC.names}
DF = [0.6, 0.25, 0.05]
SIZES = [5, 20_003]
SS_EINVAL, SS_ENOTSUP = -1, -4


@pytest.fixture(scope="module")
def S():
    import seekstorm_amd
    return seekstorm_amd


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


class World:
    pass


def _lists(n_docs, seed):
    rng = np.random.default_rng(seed)
    offs, docs, tfs = [0], [], []
    for df in DF:
        d = np.sort(rng.choice(n_docs, max(1, int(df * n_docs)), replace=False)).astype(np.uint32)
        docs.append(d); tfs.append(np.minimum(rng.geometric(0.6, len(d)), 60).astype(np.uint16)); offs.append(offs[-1] + len(d))
    return np.asarray(offs, np.uint64), np.concatenate(docs), np.concatenate(tfs)


def _records(n_docs, seed, n_words=len(WORDS)):
    rng = np.random.default_rng(seed)
    v = np.zeros(n_docs, REC)
    v["s16"] = rng.integers(0, n_words, n_docs)
    v["s32"] = rng.integers(0, n_words, n_docs)
    v["h"] = rng.integers(0, 9, n_docs)
    v["f"] = rng.normal(0.0, 50.0, n_docs).astype(np.float32)
    v["u"] = rng.permutation(n_docs)
    return v


def _raw(v):
    return np.ascontiguousarray(v.view(np.uint8).reshape(len(v), REC.itemsize))


def _np_ranks(words):
    """rank of every id's string: byte-wise order, equal strings share a rank (numpy / Python, not the library's helper)"""
    keys = [w.encode("utf-8") for w in words]
    order = sorted(set(keys))
    return np.array([order.index(kb) for kb in keys], np.int64)


def _world(S, O, n_docs):
    W = World()
    W.n = n_docs
    W.dl = O.lex_doclen(n_docs)
    W.offs, W.docs, W.tfs = _lists(n_docs, 5)
    W.v = _records(n_docs, 6)
    W.gone = sorted({d for d in (0, 63, 64, 4095, 4096, n_docs - 1) if 0 <= d < n_docs})
    W.alive = np.ones(n_docs, bool)
    W.alive[W.gone] = False
    # the shard under test: rank tables on the device
    W.sh = S.Shard(0)
    W.sh.upload_lexical(n_docs, W.dl, W.offs, W.docs, W.tfs)
    W.sh.upload_facets(_raw(W.v))
    W.sh.set_string_facet_ranks(OFF["s16"], "string16", WORDS)
    W.sh.set_string_facet_ranks(OFF["s32"], "string32", WORDS)
    W.sh.set_deleted(W.gone)
    # the existing path: two rank columns appended by the host
    raw1, W.col16 = S.Shard.string_facet_rank_column(_raw(W.v), OFF["s16"], "string16", WORDS)
    raw2, W.col32 = S.Shard.string_facet_rank_column(raw1, OFF["s32"], "string32", WORDS)
    W.host = S.Shard(0)
    W.host.upload_lexical(n_docs, W.dl, W.offs, W.docs, W.tfs)
    W.host.upload_facets(raw2)
    W.host.set_deleted(W.gone)
    W.osh = O.Shard(n_docs, W.dl, W.offs, W.docs, W.tfs)
    W.osh.set_deleted(W.gone)
    return W


@pytest.fixture(scope="module")
def worlds(S, O):
    made = {}

    def get(n_docs):
        if n_docs not in made:
            made[n_docs] = _world(S, O, n_docs)
        return made[n_docs]
    yield get
    for W in made.values():
        W.sh.close(); W.host.close()


def _string_key(kb, desc):
    return tuple(-b for b in kb) + (1,) if desc else tuple(kb) + (-1,)  # descending: reversed byte order, the longer string first


# (sort fields of the device path, the same on the host rank-column path, the brute-force key of doc d)
def _cases(W, words):
    skey = [w.encode("utf-8") for w in words]
    v = W.v
    return [
        ("s16 ascending", [(OFF["s16"], "string16", False)], [(W.col16, "u32", False)], lambda d: (_string_key(skey[int(v["s16"][d])], False),)),
        ("s16 descending", [(OFF["s16"], "string16", True)], [(W.col16, "u32", True)], lambda d: (_string_key(skey[int(v["s16"][d])], True),)),
        ("s32 ascending, h descending", [(OFF["s32"], "string32", False), (OFF["h"], "u16", True)], [(W.col32, "u32", False), (OFF["h"], "u16", True)],
         lambda d: (_string_key(skey[int(v["s32"][d])], False), -int(v["h"][d]))),
        ("s32 descending, f ascending", [(OFF["s32"], "string32", True), (OFF["f"], "f32", False)], [(W.col32, "u32", True), (OFF["f"], "f32", False)],
         lambda d: (_string_key(skey[int(v["s32"][d])], True), float(v["f"][d]))),
        ("h ascending, s16 descending", [(OFF["h"], "u16", False), (OFF["s16"], "string16", True)], [(OFF["h"], "u16", False), (W.col16, "u32", True)],
         lambda d: (int(v["h"][d]), _string_key(skey[int(v["s16"][d])], True))),
    ]


def _check_sorted(S, O, W, sh, words, host=None, ks=(10, 77, 1500), what=""):
    for terms, qt, oop in (([0, 1, 2], S.QueryType.Union, O.OP_OR), ([0, 1], S.QueryType.Intersection, O.OP_AND)):
        q = sh.make_queries([terms], qt)
        ad, as_, atot = W.osh.search_exhaustive(terms, oop, W.n)
        for name, spec, host_spec, key in _cases(W, words):
            order = sorted(range(len(ad)), key=lambda i: key(int(ad[i])) + (-float(as_[i]),))
            for k in ks:
                doc, score, tot = sh.search_lexical_sorted(q, spec, k)
                want = ad[order[:k]]
                assert tot == atot and len(doc) == len(want), (what, name, terms, k)
                # the order the strings' bytes and the other fields impose (inside their ties: by score)
                assert [key(int(d)) for d in doc] == [key(int(d)) for d in want], (what, name, terms, k)
                assert np.allclose(score, as_[order[:k]], rtol=1e-4), (what, name, terms, k)
                if host is not None:
                    hd, hs, ht = host.search_lexical_sorted(host.make_queries([terms], qt), host_spec, k)
                    assert np.array_equal(doc, hd) and np.array_equal(score.view(np.uint32), hs.view(np.uint32)) and tot == ht, (what, name, terms, k)


@pytest.mark.parametrize("n_docs", SIZES)
def test_sorted_searches_by_string_fields(S, O, worlds, n_docs):
    """ascending, descending, with a second numeric field, mixed, a numeric field first; k = 10, 77 and a deep page of 1 500"""
    W = worlds(n_docs)
    assert W.sh.facet_info() == (n_docs, REC.itemsize, n_docs, 2)
    _check_sorted(S, O, W, W.sh, WORDS, host=W.host)
    # the ranks as a merge across shards reads them
    d = np.arange(n_docs, dtype=np.uint32)
    assert np.array_equal(W.sh.string_facet_ranks(d, OFF["s16"], "string16"), _np_ranks(WORDS)[W.v["s16"]].astype(np.uint32))
    assert np.array_equal(W.sh.string_facet_ranks(d, OFF["s32"], "string32"), _np_ranks(WORDS)[W.v["s32"]].astype(np.uint32))
    assert np.array_equal(W.sh.string_facet_ranks([n_docs, 0], OFF["s16"], "string16"),
                          np.array([0xFFFFFFFF, _np_ranks(WORDS)[W.v["s16"][0]]], np.uint32))
    assert np.array_equal(W.sh.facet_values(d, OFF["s16"], "string16"), W.v["s16"].astype(np.uint64))  # ss_facet_values keeps returning ids


@pytest.mark.parametrize("n_docs", SIZES)
def test_docs_search_sorted_by_a_string_field_under_a_filter(S, worlds, n_docs):
    """the empty query: np.lexsort by (rank of the string, then the doc id, the larger first), a filter on h, pages with a skip --
    shallow and across SS_MAX_K"""
    W = worlds(n_docs)
    flt = [(OFF["h"], "u16", 2, 7)]
    docs = np.nonzero(W.alive & (W.v["h"] >= 2) & (W.v["h"] < 7))[0]
    rk = _np_ranks(WORDS)
    for spec, cols in (([(OFF["s16"], "string16", False)], [rk[W.v["s16"][docs]]]),
                       ([(OFF["s32"], "string32", True), (OFF["h"], "u16", False)], [-rk[W.v["s32"][docs]], W.v["h"][docs].astype(np.int64)])):
        order = docs[np.lexsort([-docs] + cols[::-1])]
        for skip, k in ((0, 10), (3, 20), (1000, 100)):
            d, cnt, tot, _ = W.sh.search_docs(k, S.ResultType.TopkCount, flt, spec, skip=skip)
            assert tot == len(docs) and cnt == len(order[skip:skip + k]) and np.array_equal(d, order[skip:skip + k]), (spec, skip, k)


def test_without_a_table_string_sorts_are_refused_as_before(S, worlds):
    W = worlds(SIZES[0])
    q = W.host.make_queries([[0, 1]], S.QueryType.Union)
    with pytest.raises(S.SeekStormHipError) as e:
        W.host.search_lexical_sorted(q, [(OFF["s16"], "string16", False)], 10)
    assert e.value.code == SS_ENOTSUP
    with pytest.raises(S.SeekStormHipError) as e:
        W.host.search_docs(10, result_sort=[(OFF["s16"], "string16", False)])
    assert e.value.code == SS_EINVAL
    with pytest.raises(S.SeekStormHipError):
        W.host.string_facet_ranks([0], OFF["s16"], "string16")
    with pytest.raises(S.SeekStormHipError) as e:  # the pivot entry keeps refusing string types, table or not
        W.sh.facet_kth(W.sh.make_queries([[0, 1]], S.QueryType.Union), OFF["s16"], "string16", False, 3)
    assert e.value.code == SS_ENOTSUP


def test_refused_tables_leave_the_answers_unchanged(S, O, worlds):
    from seekstorm_amd import _native as N
    W = worlds(SIZES[1])
    L, sh = N.lib(), W.sh
    d = np.arange(W.n, dtype=np.uint32)
    before = (sh.facet_info(), sh.string_facet_ranks(d, OFF["s16"], "string16"), sh.string_facet_ranks(d, OFF["s32"], "string32"))
    full = np.zeros(65536, np.uint32)
    short = np.zeros(int(W.v["s16"].max()), np.uint32)  # the largest id present is not named
    assert L.ss_facet_set_string_ranks(sh._h, OFF["s16"], N.FACET_TYPES["string16"], len(short), N.ptr(short, N.u32p)) == SS_EINVAL
    assert L.ss_facet_set_string_ranks(sh._h, OFF["h"], N.FACET_TYPES["u16"], len(full), N.ptr(full, N.u32p)) == SS_EINVAL
    assert L.ss_facet_set_string_ranks(sh._h, REC.itemsize - 1, N.FACET_TYPES["string16"], len(full), N.ptr(full, N.u32p)) == SS_EINVAL
    assert L.ss_facet_set_string_ranks(sh._h, OFF["s16"], N.FACET_TYPES["string16"], 4, None) == SS_EINVAL
    assert L.ss_facet_set_string_ranks(None, OFF["s16"], N.FACET_TYPES["string16"], len(full), N.ptr(full, N.u32p)) == SS_EINVAL
    # six more tables fill the eight (a String16 facet at any offset holds ids below 65 536); the ninth is refused
    extra = [o for o in range(REC.itemsize - 1) if o != OFF["s16"]][:N.SS_MAX_STRING_RANKS - 2]
    for o in extra:
        assert L.ss_facet_set_string_ranks(sh._h, o, N.FACET_TYPES["string16"], len(full), N.ptr(full, N.u32p)) == 0
    assert sh.facet_info()[3] == N.SS_MAX_STRING_RANKS
    assert L.ss_facet_set_string_ranks(sh._h, REC.itemsize - 2, N.FACET_TYPES["string16"], len(full), N.ptr(full, N.u32p)) == SS_ENOTSUP
    for o in extra:  # forgotten again
        assert L.ss_facet_set_string_ranks(sh._h, o, N.FACET_TYPES["string16"], 0, None) == 0
    after = (sh.facet_info(), sh.string_facet_ranks(d, OFF["s16"], "string16"), sh.string_facet_ranks(d, OFF["s32"], "string32"))
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and np.array_equal(before[2], after[2])
    _check_sorted(S, O, W, sh, WORDS, ks=(77,), what="after refusals")


def test_commits_extend_the_rank_columns(S, O):
    """a level of known strings: the sort covers its docs.  A level holding an id beyond the table: SS_EINVAL, nothing changed.  A new
    table whose new string sorts FIRST -- the empty string, which this test's first word list therefore leaves out: every old rank
    moves -- and then the level: brute force again.  The levels are commits of level 0 growing from 12 000 to 16 000 to 20 003 docs."""
    from seekstorm_amd import _native as N
    n0, n1, n2 = 12_000, 16_000, SIZES[1]
    W = World()
    W.n = n2
    W.dl = O.lex_doclen(n2)
    W.offs, W.docs, W.tfs = _lists(n2, 5)
    W.v = _records(n2, 6)
    W.col16 = W.col32 = 0
    words1 = [w or "c" for w in WORDS]
    words2 = words1 + [""]
    new_id = len(WORDS)
    W.v["s16"][n1:n2:3] = new_id  # the last level brings the new string
    W.v["s32"][n1 + 1:n2:5] = new_id
    raw = _raw(W.v)

    def csr(n):
        o, d, t = [0], [], []
        for i in range(len(DF)):
            a, b = int(W.offs[i]), int(W.offs[i + 1])
            i1 = a + int(np.searchsorted(W.docs[a:b], n))
            d.append(W.docs[a:i1]); t.append(W.tfs[a:i1]); o.append(o[-1] + (i1 - a))
        return np.asarray(o, np.uint64), np.concatenate(d), np.concatenate(t)

    def at(n):  # the world cut to the docs committed so far
        V = World()
        V.n, V.v, V.col16, V.col32 = n, W.v[:n], 0, 0
        V.osh = O.Shard(n, W.dl[:n], *csr(n))
        return V

    sh = S.Shard(0)
    try:
        sh.reserve_facets(n1)  # the second commit fits, the third must move image AND columns
        sh.append_facet_level(0, raw[:n0])
        sh.append_level(0, W.dl[:n0], *csr(n0))
        sh.set_string_facet_ranks(OFF["s16"], "string16", words1)
        sh.set_string_facet_ranks(OFF["s32"], "string32", words1)
        _check_sorted(S, O, at(n0), sh, words1, ks=(77,), what="first commit")
        sh.append_facet_level(0, raw[:n1])
        sh.append_level(0, W.dl[:n1], *csr(n1))
        assert sh.facet_info() == (n1, REC.itemsize, n1, 2)
        _check_sorted(S, O, at(n1), sh, words1, ks=(77, 1500), what="a level of known strings")
        # an id beyond the table
        d = np.arange(n1, dtype=np.uint32)
        before = (sh.facet_info(), sh.string_facet_ranks(d, OFF["s16"], "string16"), sh.facet_values(d, OFF["s32"], "string32"))
        assert N.lib().ss_facet_append_level(sh._h, 0, n2, REC.itemsize, N.ptr(raw, N.u8p)) == SS_EINVAL
        assert sh.facet_info() == before[0] and np.array_equal(sh.string_facet_ranks(d, OFF["s16"], "string16"), before[1])
        assert np.array_equal(sh.facet_values(d, OFF["s32"], "string32"), before[2])
        _check_sorted(S, O, at(n1), sh, words1, ks=(77,), what="after the refused level")
        # the table for the new id space first, then the level
        sh.set_string_facet_ranks(OFF["s16"], "string16", words2)
        sh.set_string_facet_ranks(OFF["s32"], "string32", words2)
        assert np.array_equal(sh.string_facet_ranks(d, OFF["s16"], "string16"), _np_ranks(words2)[W.v["s16"][:n1]].astype(np.uint32))
        assert _np_ranks(words2)[new_id] == 0 and (_np_ranks(words2)[:new_id] == _np_ranks(words1) + 1).all()  # every old rank moved
        sh.append_facet_level(0, raw)
        sh.append_level(0, W.dl, *csr(n2))
        assert sh.facet_info() == (n2, REC.itemsize, n1 + n1 // 2, 2)
        _check_sorted(S, O, at(n2), sh, words2, ks=(77, 1500), what="new strings")
        dd = np.arange(n2, dtype=np.uint32)
        assert np.array_equal(sh.string_facet_ranks(dd, OFF["s32"], "string32"), _np_ranks(words2)[W.v["s32"]].astype(np.uint32))
    finally:
        sh.close()


@pytest.mark.parametrize("n_held,level,n_level", [(4096, 0, 4097), (65536, 1, 5)])
def test_a_level_beyond_the_only_table_is_refused_at_odd_sizes(S, n_held, level, n_level):
    """ONE registered table and an odd number of docs in the level -- the ordinary shape of a partial level of a shard with one string
    facet: a level in which one doc holds an id >= n_ids is refused with SS_EINVAL and facet_info, every stored value and every rank
    stay; the same level without that id is accepted and ranked"""
    from seekstorm_amd import _native as N
    n = level * 65536 + n_level
    v = _records(n, 21)
    raw = _raw(v)
    bad = raw.copy()
    bad.view(REC)["s16"][n - 2, 0] = len(WORDS)  # (the last but one doc of the level)
    sh = S.Shard(0)
    try:
        sh.append_facet_level(0, raw[:n_held])
        sh.set_string_facet_ranks(OFF["s16"], "string16", WORDS)
        d = np.arange(n_held, dtype=np.uint32)
        before = (sh.facet_info(), sh.string_facet_ranks(d, OFF["s16"], "string16"), [sh.facet_values(d, OFF[c], t) for c, t in (("s16", "string16"), ("u", "u32"))])
        assert before[0] == (n_held, REC.itemsize, n_held, 1)
        lo = level * 65536
        assert N.lib().ss_facet_append_level(sh._h, level, n_level, REC.itemsize, N.ptr(np.ascontiguousarray(bad[lo:n]), N.u8p)) == SS_EINVAL
        assert sh.facet_info() == before[0]
        assert np.array_equal(sh.string_facet_ranks(d, OFF["s16"], "string16"), before[1])
        assert all(np.array_equal(sh.facet_values(d, OFF[c], t), b) for (c, t), b in zip((("s16", "string16"), ("u", "u32")), before[2]))
        sh.append_facet_level(level, raw[lo:n])
        dd = np.arange(n, dtype=np.uint32)
        assert sh.facet_info()[:2] == (n, REC.itemsize) and sh.facet_info()[3] == 1
        assert np.array_equal(sh.string_facet_ranks(dd, OFF["s16"], "string16"), _np_ranks(WORDS)[v["s16"]].astype(np.uint32))
        assert np.array_equal(sh.facet_values(dd, OFF["u"], "u32"), v["u"].astype(np.uint64))
    finally:
        sh.close()


def _two_shard_corpus(O):
    """a corpus split over two shards with their OWN value ids: (whole-corpus records and word list, per shard the lexical CSR, records
    and word list)"""
    n_docs, S_n = SIZES[1], 2
    dl = O.lex_doclen(n_docs)
    offs, docs, tfs = _lists(n_docs, 5)
    rng = np.random.default_rng(9)
    # the shards' own id spaces: each a shuffle of the words plus a word only that shard knows
    lists = [[str(w) for w in rng.permutation(WORDS)] + ["only-0"], [str(w) for w in rng.permutation(WORDS)] + ["é only-1"]]
    whole_words = sorted(set(lists[0]) | set(lists[1]), key=lambda w: (len(w), w))  # any order: ids are arbitrary
    v = _records(n_docs, 6)
    local = np.array([rng.integers(0, len(lists[g % S_n])) for g in range(n_docs)], np.uint32)
    v["s16"] = [whole_words.index(lists[g % S_n][local[g]]) for g in range(n_docs)]
    v["s32"] = v["s16"]
    parts = []
    for sid in range(S_n):  # doc g -> shard g % S, local id g // S (index.rs:5284)
        sel = np.arange(sid, n_docs, S_n)
        o2, d2, t2 = [0], [], []
        for t in range(len(DF)):
            d = docs[int(offs[t]):int(offs[t + 1])]
            f = tfs[int(offs[t]):int(offs[t + 1])]
            m = (d % S_n) == sid
            d2.append(d[m] // S_n); t2.append(f[m]); o2.append(o2[-1] + int(m.sum()))
        vs = v[sel].copy()
        vs["s16"] = local[sel]; vs["s32"] = local[sel]
        parts.append((len(sel), np.ascontiguousarray(dl[sel]), np.asarray(o2, np.uint64), np.concatenate(d2).astype(np.uint32), np.concatenate(t2), _raw(vs)))
    return (n_docs, dl, offs, docs, tfs, _raw(v), whole_words), parts, lists


TWO_SHARD_SORTS = ([(OFF["s16"], "string16", False), (OFF["u"], "u32", True)], [(OFF["s32"], "string32", True), (OFF["u"], "u32", False)])
TWO_SHARD_PAGES = ((0, 25, None), (7, 10, [(OFF["u"], "u32", 500, 15_000)]))


def test_index_two_shards_sorted_by_a_string_field(S, O):
    """Index.set_string_facet_ranks: every shard has its OWN value ids; one rank order over the union of the shards' strings makes the
    shards' ranks comparable, and Index.search(result_sort=[string, ...]) equals one shard holding the whole corpus.  A unique second
    field decides the ties of the strings (shard-local idf changes scores, not the order), as test_index_two_shards_result_sort has it."""
    (n_docs, dl, offs, docs, tfs, raw, whole_words), parts, lists = _two_shard_corpus(O)
    whole = S.Shard(0)
    whole.upload_lexical(n_docs, dl, offs, docs, tfs)
    whole.upload_facets(raw)
    for name, ty in (("s16", "string16"), ("s32", "string32")):
        whole.set_string_facet_ranks(OFF[name], ty, whole_words)
    shards = []
    for sid, (n, dls, o2, d2, t2, rs_) in enumerate(parts):
        sh = S.Shard(0, shard_id=sid)
        sh.upload_lexical(n, dls, o2, d2, t2)
        sh.upload_facets(rs_)
        shards.append(sh)
    try:
        idx = S.Index(shards)
        idx.set_string_facet_ranks(OFF["s16"], "string16", lists)
        idx.set_string_facet_ranks(OFF["s32"], "string32", lists)
        for terms, qt in (([0, 1, 2], S.QueryType.Union), ([0, 1], S.QueryType.Intersection)):
            q = whole.make_queries([terms], qt)
            for sort in TWO_SHARD_SORTS:
                for off_, length, flt in TWO_SHARD_PAGES:
                    wd, ws, wtot = whole.search_lexical_sorted(q, sort, off_ + length, facet_filter=flt)
                    ro = idx.search(terms, None, qt, S.SearchMode.Lexical, off_, length, strict=True, facet_filter=flt, result_sort=sort)
                    assert ro.result_count_total == wtot
                    assert [r.doc_id for r in ro.results] == [int(x) for x in wd[off_:off_ + length]], (terms, sort, off_, length)
    finally:
        for sh in shards + [whole]:
            sh.close()


def test_cpp_mirror_sorts_two_shards_by_a_string_field(S, O):
    """the C++ mirror: Index::set_string_facet_ranks + Index::search_lexical_sorted over two shards built by commits of the facet image
    (Shard::append_facet_level) and tombstones added in place (Shard::add_deleted) -- against one Python shard holding the whole corpus"""
    import ctypes as C
    from seekstorm_amd import _native as N
    from host_mirror import HOST_LIB, P, SortC as _SortC, f32p, u8p, u16p, u32p, u64p
    N.lib()
    H = C.CDLL(HOST_LIB)
    H.ssh_index_create.restype = C.c_void_p
    H.ssh_index_create.argtypes = [C.c_int, C.POINTER(C.c_int)]
    H.ssh_index_destroy.argtypes = [C.c_void_p]
    H.ssh_upload_lexical.argtypes = [C.c_void_p, C.c_int, C.c_uint64, u8p, C.c_uint32, u64p, u32p, u16p]
    H.ssh_append_facet_level.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
    H.ssh_reserve_facets.argtypes = [C.c_void_p, C.c_int, C.c_uint64]
    H.ssh_facet_info.argtypes = [C.c_void_p, C.c_int, u64p, u32p, u64p, u32p]
    H.ssh_add_deleted.argtypes = [C.c_void_p, C.c_int, u64p, C.c_uint64]
    H.ssh_index_set_string_facet_ranks.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_char_p, C.c_uint64, u32p]
    H.ssh_string_facet_ranks.argtypes = [C.c_void_p, C.c_int, u32p, C.c_uint32, C.c_uint32, C.c_uint32, u32p]
    H.ssh_index_search_sorted.argtypes = [C.c_void_p, u32p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                          C.c_uint32, C.c_uint32, u64p, f32p, u64p]
    (n_docs, dl, offs, docs, tfs, raw, whole_words), parts, lists = _two_shard_corpus(O)
    gone = [0, 1, 63, 64, 4095, 4096, n_docs - 1]  # global ids: doc g lives in shard g % 2 as g // 2
    whole = S.Shard(0)
    ix = H.ssh_index_create(2, None)
    try:
        whole.upload_lexical(n_docs, dl, offs, docs, tfs)
        whole.upload_facets(raw)
        for name, ty in (("s16", "string16"), ("s32", "string32")):
            whole.set_string_facet_ranks(OFF[name], ty, whole_words)
        whole.set_deleted(gone[:2])
        whole.add_deleted(gone[2:])
        for sid, (n, dls, o2, d2, t2, rs_) in enumerate(parts):
            assert H.ssh_upload_lexical(ix, sid, n, P(dls, u8p), len(DF), P(o2, u64p), P(d2, u32p), P(t2, u16p)) == 0
            assert H.ssh_reserve_facets(ix, sid, n) == 0
            half = n // 2
            assert H.ssh_append_facet_level(ix, sid, 0, half, REC.itemsize, rs_.ctypes.data) == 0  # level 0, partial, then re-committed whole
            assert H.ssh_append_facet_level(ix, sid, 0, n, REC.itemsize, rs_.ctypes.data) == 0
            nd, rs, cap, nt = C.c_uint64(), C.c_uint32(), C.c_uint64(), C.c_uint32()
            assert H.ssh_facet_info(ix, sid, C.byref(nd), C.byref(rs), C.byref(cap), C.byref(nt)) == 0
            assert (nd.value, rs.value, cap.value, nt.value) == (n, REC.itemsize, n, 0)
            local_gone = np.array([g // 2 for g in gone if g % 2 == sid], np.uint64)
            assert H.ssh_add_deleted(ix, sid, P(local_gone, u64p), len(local_gone)) == 0
        blob = b"\0".join(w.encode("utf-8") for ws in lists for w in ws)
        counts = np.array([len(ws) for ws in lists], np.uint32)
        for name, ty in (("s16", "string16"), ("s32", "string32")):
            assert H.ssh_index_set_string_facet_ranks(ix, OFF[name], N.FACET_TYPES[ty], blob, len(blob), P(counts, u32p)) == 0
        # the shards' ranks are those of the one order over all strings
        order = sorted({w.encode("utf-8") for ws in lists for w in ws})
        for sid, (n, _, _, _, _, rs_) in enumerate(parts):
            d = np.arange(n, dtype=np.uint32)
            out = np.zeros(n, np.uint32)
            assert H.ssh_string_facet_ranks(ix, sid, P(d, u32p), n, OFF["s16"], N.FACET_TYPES["string16"], P(out, u32p)) == 0
            ids = rs_.view(REC)["s16"][:, 0]
            assert np.array_equal(out, np.array([order.index(lists[sid][int(i)].encode("utf-8")) for i in ids], np.uint32))
        for terms, qt in (([0, 1, 2], 1), ([0, 1], 0)):
            q = whole.make_queries([terms], S.QueryType(qt))
            for sorts in TWO_SHARD_SORTS:
                for off_, length, flt in TWO_SHARD_PAGES:
                    wd, ws, wtot = whole.search_lexical_sorted(q, list(sorts), off_ + length, facet_filter=flt)
                    sarr = (_SortC * len(sorts))()
                    for i, so in enumerate(sorts):
                        sarr[i].facet_offset, sarr[i].facet_type, sarr[i].descending = so[0], N.FACET_TYPES[so[1]], 1 if so[2] else 0
                    farr, nf = S.Shard.facet_filters(flt) if flt else (None, 0)
                    t = np.ascontiguousarray(terms, np.uint32)
                    doc = np.zeros(length + 1, np.uint64); sc = np.zeros(length + 1, np.float32); meta = np.zeros(4, np.uint64)
                    n = H.ssh_index_search_sorted(ix, P(t, u32p), len(t), qt, off_, length, nf, None if farr is None else C.cast(farr, C.c_void_p),
                                                  C.cast(sarr, C.c_void_p), len(sorts), length + 1, P(doc, u64p), P(sc, f32p), P(meta, u64p))
                    assert int(meta[3]) == 0 and int(meta[1]) == wtot
                    assert [int(x) for x in doc[:n]] == [int(x) for x in wd[off_:off_ + length]], (terms, sorts, off_, length)
    finally:
        H.ssh_index_destroy(ix)
        whole.close()
