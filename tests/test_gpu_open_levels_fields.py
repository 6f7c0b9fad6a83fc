"""index.bin of SEVERAL indexed fields opened LEVEL BY LEVEL, its field vectors decoded on the device, ready for commit_level_fields
(ss_bm25_open_index_bin_levels_fields / Shard.open_index_bin_levels_fields, ss_bm25_level_read_fields / Shard.read_level_fields).

One seeded corpus of 3 * 65536 + 500 docs over 3 fields (boosts 2, 1, 0.5), about 40 terms shaped so that real levels of the file hold
Arrays of 1, 63, 64, 65 and 4095 postings, an Rle ending at doc 65 535, a full level, a Bitmap, a term absent from a level, a term only in
the last level, a term living in one field only, docs holding a term in all three fields, 2-byte and 3-byte pointers (a lowered
positions_limit), one bigram and one trigram key.  index.bin is written from the first 2 * 65536 + 1000 docs: its last level is partial.

For positions off (the device decoder) and "host":
  1. the opened shard answers a fixed query set exactly as a shard given upload_index_bin of the same file;
  2. read_level_fields of every level equals the numpy restatement of mf_level_prepare over the corpus, the read-back of a shard that got
     the same levels through commit_level_fields, and (postings arrays) the other mode's levels;
  3. the life cycle: level 2 re-committed with the docs up to 3 * 65536, level 3 committed with the last 500 docs and a new term -- after
     each step the answers equal those of a fresh shard given one upload_lexical_fields of the same prefix;
  4. files with one in-bounds defect, which the host decoder refuses too (checked here through ss_ref_decode_block_fields), a tiered ix,
     mode "device" and a one-field file are refused and the shard keeps its levels and answers;
  5. one-level files of 2 and of 8 fields whose postings hold every embedded tag that valid positions can make.
The format defines every embedded tag (0x8 .. 0xF, 0x10 .. 0x1F), so "an unknown tag" cannot be written: the defect in its place is an
embedded pointer whose field slot names a field the index does not have."""
import ctypes as C

import numpy as np
import pytest

from oracle import ref_format as RF

pytestmark = pytest.mark.gpu

LV = 65536
N_FULL = 3 * LV + 500
N_FILE = 2 * LV + 1000
HEAD = 23
LIMIT = 2000
F3 = 3
LONGEST = 1
BOOST = [2.0, 1.0, 0.5]
MODES = [False, "host"]


@pytest.fixture(scope="module")
def S():
    import seekstorm_amd
    return seekstorm_amd


@pytest.fixture(scope="module")
def N():
    from seekstorm_amd import _native
    return _native


class _List:
    """one term id: entries (doc, field, tf) sorted by (doc, field), npos positions behind each (the tf, except for the component lists of
    an n-gram key: the key's own count behind component 0's entries, none behind the others)"""

    def __init__(self, key, comp, docs, fields, tfs, npos, pos):
        self.key, self.comp = int(key), int(comp)
        self.docs, self.fields = np.asarray(docs, np.uint32), np.asarray(fields, np.uint8)
        self.tfs, self.npos, self.pos = np.asarray(tfs, np.uint16), np.asarray(npos, np.uint16), np.asarray(pos, np.uint16)
        self.pstart = np.concatenate(([0], np.cumsum(self.npos.astype(np.int64))))
        k = self.docs.astype(np.int64) * 16 + self.fields
        assert np.all(np.diff(k) > 0) and len(self.pos) == self.pstart[-1] and np.all(self.tfs > 0)

    def cut(self, lo, hi):
        return int(np.searchsorted(self.docs, lo)), int(np.searchsorted(self.docs, hi))


def _positions(rng, counts, max_gap=6):
    counts = np.asarray(counts, np.int64)
    tot = int(counts.sum())
    gaps = rng.integers(0, max_gap, tot).astype(np.int64) + 1
    c = np.cumsum(gaps)
    starts = np.cumsum(counts) - counts
    base = np.repeat(c[starts[counts > 0]] - gaps[starts[counts > 0]], counts[counts > 0])
    return (c - base - 1).astype(np.uint16)


def _per_entry(l, i1=None):
    i1 = len(l.docs) if i1 is None else i1
    return [[int(x) for x in l.pos[l.pstart[i]:l.pstart[i + 1]]] for i in range(i1)]


class _Corpus:
    def __init__(self, n_fields=F3, longest=LONGEST):
        rng = np.random.default_rng(616)
        self.rng, self.F, self.longest = rng, n_fields, longest
        F = n_fields
        self.doclen = rng.integers(1, 120, (F, N_FULL)).astype(np.uint8)
        self.single, self.ngram, self.names = [], [], {}
        used = set()

        def key(ntype=0):
            while True:
                k = (int(rng.integers(1, 1 << 60)) << 3) | ntype
                if k not in used:
                    used.add(k)
                    return k
        self._key = key

        def at(level, local):
            return [level * LV + int(x) for x in local]

        def entries(docs, mode, tf=None):
            """mode: "rand" a random non-empty subset of the fields per doc, "all" every field, an int that field only"""
            docs = np.asarray(sorted(docs), np.int64)
            if mode == "rand":
                mask = rng.integers(1, 1 << F, len(docs))
            elif mode == "all":
                mask = np.full(len(docs), (1 << F) - 1)
            else:
                mask = np.full(len(docs), 1 << mode)
            d = np.concatenate([docs[(mask >> f) & 1 == 1] for f in range(F)])
            fl = np.concatenate([np.full(int(((mask >> f) & 1).sum()), f) for f in range(F)])
            o = np.lexsort((fl, d))
            d, fl = d[o], fl[o]
            tfs = np.minimum(rng.geometric(0.5, len(d)), 5) if tf is None else np.full(len(d), tf)
            return d, fl, tfs

        def term(name, docs, mode="rand", tf=None):
            d, fl, tfs = entries(docs, mode, tf)
            l = _List(key(), 0, d, fl, tfs, tfs, _positions(rng, tfs))
            self.single.append(l)
            self.names[name] = l
            return l

        spaced = lambda n, step=3, first=1: [first + step * i for i in range(n)]
        term("a1", at(0, [777]) + at(1, spaced(100, 50)))
        for n in (63, 64, 65):
            term(f"a{n}", at(0, spaced(n, 11)) + at(2, [10, 500, 999, 1200]))
        term("a4095", at(1, spaced(4095, 16)))
        term("rle_one", at(0, range(1000, 1300)), LONGEST, tf=1)
        term("rle_end", at(0, [7] + list(range(65000, 65536))) + at(1, range(0, 50)))
        term("rle_full", at(1, range(LV)) + at(2, range(1500)), LONGEST, tf=1)
        term("bm_bits", at(0, sorted({63, 64, 65535} | {int(x) for x in rng.choice(np.arange(0, 65535, 5), 4200, replace=False)})))
        term("absent1", at(0, spaced(100, 31)) + at(2, spaced(30, 60)))
        term("only_last", at(2, spaced(80, 12) + spaced(100, 400, 1003)))
        term("one_field", rng.choice(N_FULL, 600, replace=False), 2)
        term("all3", rng.choice(N_FULL, 500, replace=False), "all")
        # records of known bytes for the defects: field 2 with 5 positions (one byte 0xA0 | 5 << 2 | 2); fields 0 and 2 with 5 each; an
        # embedded pointer of field 0 (tag 0x8)
        term("rec_f2", at(0, spaced(20, 7)), 2, tf=5)
        term("rec_two", at(0, spaced(20, 9)), "rand", tf=5)
        l = self.names["rec_two"]
        d = np.repeat(np.unique(l.docs), 2)
        self.single[-1] = self.names["rec_two"] = _List(l.key, 0, d, np.tile([0, 2], len(d) // 2), np.full(len(d), 5), np.full(len(d), 5),
                                                       _positions(rng, np.full(len(d), 5)))
        term("emb_f0", at(0, spaced(20, 13)), 0, tf=1)
        for i, df in enumerate((0.001, 0.003, 0.01, 0.03, 0.08)):
            term(f"m{i}", rng.choice(N_FULL, int(df * N_FULL), replace=False))
        for i in range(12):
            term(f"r{i}", {int(rng.integers(0, N_FILE))} | set(int(x) for x in rng.integers(0, N_FULL, int(rng.integers(1, 30)))))
        # ---- one bigram and one trigram key: the components' field vectors in front of the key's own
        for name, ntype, n in (("ng2", 1, 80), ("ng3", 4, 70)):
            nc = 2 if ntype <= 3 else 3
            docs = np.sort(rng.choice(N_FILE, n, replace=False))
            od, ofl, ocnt = entries(docs, "rand")
            own = {}
            for d_, f_, c_ in zip(od, ofl, ocnt):
                own.setdefault(int(d_), {})[int(f_)] = int(c_)
            vecs, comp = {}, [[] for _ in range(nc)]
            for d_ in docs:
                d_ = int(d_)
                vecs[d_] = []
                for c in range(nc):
                    fs = set(own[d_]) if c == 0 else set()
                    fs |= {int(x) for x in rng.choice(F, int(rng.integers(1, F + 1)), replace=False)}
                    v = [(f, max(own[d_].get(f, 0) if c == 0 else 0, int(rng.choice([1, 2, 90, 300, 17000])))) for f in sorted(fs)]
                    vecs[d_].append(v)
                    comp[c] += [(d_, f, tf, own[d_].get(f, 0) if c == 0 else 0) for f, tf in v]
            opos = _positions(rng, ocnt)
            k = key(ntype)
            lists = []
            for c in range(nc):
                e = np.asarray(comp[c], np.int64)
                lists.append(_List(k, c, e[:, 0], e[:, 1], e[:, 2], e[:, 3], opos if c == 0 else np.zeros(0, np.uint16)))
            self.ngram.append((k, lists, od, ofl, ocnt, vecs, opos))
            self.names[name] = lists
        d, fl, tfs = entries(at(3, spaced(150, 3)), "rand")
        self.new_term = _List(key(), 0, d, fl, tfs, tfs, _positions(rng, tfs))
        self.file = self._write()

    def _write(self):
        terms, ngram_terms = [], []
        for l in self.single:
            _, i1 = l.cut(0, N_FILE)
            assert i1 > 0
            terms.append((l.key, l.docs[:i1].astype(np.int64), l.fields[:i1].astype(np.int64), l.tfs[:i1], _per_entry(l, i1)))
        for k, lists, od, ofl, ocnt, vecs, opos in self.ngram:
            own = _List(k, 0, od, ofl, ocnt, ocnt, opos)
            ngram_terms.append((k, od, ofl, ocnt, vecs, [40 + c for c in range(len(lists))], _per_entry(own)))
        return RF.write_index_bin(N_FILE, self.doclen[:, :N_FILE], terms, self.rng, key_head_size=HEAD, positions_limit=LIMIT, n_fields=self.F,
                                  longest_field_id=self.longest, ngram_terms=ngram_terms)

    def lists_of(self, ix):
        every = list(self.single) + [l for _, lists, *_ in self.ngram for l in lists]
        ids = {}
        for l in every:
            t = ix.term_of_key(l.key)
            assert t is not None
            ids[t + l.comp] = l
        assert sorted(ids) == list(range(ix.term_count))
        return [ids[t] for t in range(ix.term_count)]

    def term_id(self, order, name):
        l = self.names[name]
        return order.index(l[0]) if isinstance(l, list) else order.index(l)


@pytest.fixture(scope="module")
def corpus():
    return _Corpus()


def _csr(lists, lo, hi, stand_in=False):
    """(offs, docs, fields, tfs, npos, positions) of the lists' entries with lo <= doc < hi; stand_in: tf stand-in positions where a list's
    entries do not carry tf positions each (n-gram component lists, for an upload that takes tf positions per entry)"""
    offs, docs, fields, tfs, npos, pos = [0], [], [], [], [], []
    for l in lists:
        i0, i1 = l.cut(lo, hi)
        offs.append(offs[-1] + i1 - i0)
        docs.append(l.docs[i0:i1]); fields.append(l.fields[i0:i1]); tfs.append(l.tfs[i0:i1])
        if stand_in and not np.array_equal(l.npos, l.tfs):
            t = l.tfs[i0:i1].astype(np.int64)
            npos.append(l.tfs[i0:i1])
            pos.append((np.arange(int(t.sum())) - np.repeat(np.cumsum(t) - t, t)).astype(np.uint16))
        else:
            npos.append(l.npos[i0:i1]); pos.append(l.pos[l.pstart[i0]:l.pstart[i1]])
    cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dt)
    return np.asarray(offs, np.uint64), cat(docs, np.uint32), cat(fields, np.uint8), cat(tfs, np.uint16), cat(npos, np.uint16), cat(pos, np.uint16)


def _expected_level(lists, doclen, level, hi, F, positions):
    """mf_level_prepare (csrc/mf_level.h) restated: what a level of the lists' entries with level * 65536 <= doc < hi holds"""
    lo = level * LV
    foff, moff, tpos = [0], [0], [0]
    fdoc, ftf, mdoc, mtf, mnpos, pos = [], [], [], [], [], []
    for l in lists:
        i0, i1 = l.cut(lo, hi)
        d, fl, tf, npz = l.docs[i0:i1], l.fields[i0:i1], l.tfs[i0:i1], l.npos[i0:i1].astype(np.int64)
        for f in range(F):
            m = fl == f
            fdoc.append(d[m]); ftf.append(tf[m])
            foff.append(foff[-1] + int(m.sum()))
        u, inv = np.unique(d, return_inverse=True)
        row = np.zeros((len(u), F), np.uint16)
        row[inv, fl] = tf
        mdoc.append(u); mtf.append(row)
        moff.append(moff[-1] + len(u))
        mnpos.append(np.bincount(inv, weights=npz, minlength=len(u)).astype(np.uint32) if len(u) else np.zeros(0, np.uint32))
        p = l.pos[l.pstart[i0]:l.pstart[i1]].astype(np.uint32)
        pos.append((np.repeat(fl.astype(np.uint32), npz) << 20) | p)
        tpos.append(tpos[-1] + len(p))
    cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dt)
    out = {"foff": np.asarray(foff, np.uint64), "fdoc": cat(fdoc, np.uint32), "ftf": cat(ftf, np.uint16), "moff": np.asarray(moff, np.uint64),
           "mdoc": cat(mdoc, np.uint32), "mtf": np.concatenate(mtf).reshape(-1, F), "doclen": np.ascontiguousarray(doclen[:, lo:hi])}
    out.update({"mnpos": cat(mnpos, np.uint32), "tpos": np.asarray(tpos, np.uint64), "pos": cat(pos, np.uint32)} if positions else
               {"mnpos": None, "tpos": None, "pos": None})
    return out


POSTINGS = ("foff", "fdoc", "ftf", "moff", "mdoc", "mtf", "doclen")


def _same_level(a, b, what, keys=POSTINGS + ("mnpos", "tpos", "pos")):
    for k in keys:
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, (what, k)
        else:
            assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), (what, k)


def _query_set(S, corpus, order, positions, extra=()):
    T = lambda name: corpus.term_id(order, name)
    m = [T(f"m{i}") for i in range(5)]
    r = [T(f"r{i}") for i in (0, 3, 7, 11)]
    crafted = [T(n) for n in ("a1", "a63", "a64", "a65", "a4095", "rle_one", "rle_end", "rle_full", "bm_bits", "absent1", "only_last", "one_field", "all3",
                              "rec_f2", "rec_two", "emb_f0", "ng2", "ng3")]
    singles = [[t] for t in crafted + m + r + list(extra)]
    pairs = [[m[4], m[3]], [m[3], m[2]], [T("rle_full"), m[4]], [T("bm_bits"), T("rle_end")], [T("a4095"), T("rle_full")], [T("one_field"), m[4]],
             [T("all3"), m[4]], [T("only_last"), T("rle_full")], [T("absent1"), T("a63")], [m[4], r[0]], [T("ng2"), m[4]], [m[3], T("ng3")]]
    triples = [[m[4], m[3], m[2]], [m[0], m[1], m[2]], [T("a1"), T("a63"), T("a64")], [T("rle_one"), T("rle_end"), T("bm_bits")], [T("all3"), T("one_field"), m[4]],
               [T("only_last"), r[1], r[2]]]
    nots = [([m[4], m[3]], [m[2]]), ([m[4]], [T("rle_full")]), ([T("bm_bits"), m[3]], [m[4]]), ([T("all3")], [T("one_field"), m[4]])]
    out = []
    for qt in (S.QueryType.Union, S.QueryType.Intersection):
        for ff in (None, [1], [0, 2]):
            out.append((singles + pairs + triples if qt == S.QueryType.Union else pairs + triples, qt, None, ff))
        out.append(([a for a, _ in nots], qt, [b for _, b in nots], None))
    if positions:
        phrases = [[m[4], m[3]], [m[3], m[4]], [T("rle_full"), m[4]], [m[4], T("rle_full")], [m[4], m[3], m[2]], [T("all3"), m[4]], [T("rle_full"), T("rle_full")]]
        for ff in ([1], [0], None):
            out.append((phrases, S.QueryType.Phrase, None, ff))
    return out


def _answers(S, N, sh, sets):
    out = []
    for terms, qt, nots, ff in sets:
        q = sh.make_queries(terms, qt, nots, field_filter=ff)
        for k, rt in ((10, S.ResultType.TopkCount), (100, S.ResultType.TopkCount), (10, S.ResultType.Count)):
            try:
                out.append(tuple(np.copy(x) for x in sh.search_lexical_batch(q, k, rt, reference_shortcuts=False)))
            except N.SeekStormHipError as e:
                out.append(("refused", e.code))
    return out


def _assert_same(a, b, what, must_answer=True):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert type(x[0]) is type(y[0]), (what, i, x[:2], y[:2])
        if isinstance(x[0], str):
            assert not must_answer and x == y, (what, i, x, y)
            continue
        for u, v, name in zip(x, y, ("doc", "score", "count", "total")):
            u, v = (u.view(np.uint32), v.view(np.uint32)) if name == "score" else (u, v)
            assert np.array_equal(u, v), (what, i, name, np.argwhere(u != v)[:4].tolist())


def _index_bin(S, data, F=F3):
    return S.IndexBin(data, key_head_size=HEAD, indexed_field_count=F)


@pytest.mark.parametrize("positions", MODES)
def test_opened_levels_answer_as_the_uploaded_file(S, N, corpus, positions):
    ix = _index_bin(S, corpus.file)
    assert ix.level_count == 3 and ix.indexed_doc_count == N_FILE
    order = corpus.lists_of(ix)
    assert 35 <= len(order) <= 45
    a, b = S.Shard(0), S.Shard(0)
    try:
        a.open_index_bin_levels_fields(ix, BOOST, positions=positions)
        b.upload_index_bin(ix, BOOST, positions=bool(positions))
        assert a.incremental_info()[0] == 3 and a.lexical_field_count == 3
        info = a.open_info()
        n_post = sum(len(np.unique(l.docs[:l.cut(0, N_FILE)[1]])) for l in order)
        assert info[0] == (2 if positions else 0) and info[1] == (0 if positions else n_post) and (info[3] > 0) == bool(positions)
        sets = _query_set(S, corpus, order, positions)
        got, want = _answers(S, N, a, sets), _answers(S, N, b, sets)
        _assert_same(got, want, "open_index_bin_levels_fields against upload_index_bin")
        assert all(int(x[3].min()) > 0 for x in want[:3])  # (every single term is found)
        if positions:
            assert sum(int(x[3].sum()) for x in want[-9:]) > 0  # (some phrase matches)
    finally:
        a.close(); b.close(); ix.close()


@pytest.fixture(scope="module")
def level_reads(S, corpus):
    """{mode: [level dict]} of the opened file, shared by the tests that compare them"""
    out = {}
    ix = _index_bin(S, corpus.file)
    for positions in MODES:
        sh = S.Shard(0)
        try:
            sh.open_index_bin_levels_fields(ix, BOOST, positions=positions)
            out[positions] = [sh.read_level_fields(l, 0, ix.term_count) for l in range(3)]
            if not positions:  # a range of terms: relative offsets
                part = sh.read_level_fields(1, 3, 9)
                whole = out[positions][1]
                e0, e1, m0, m1 = int(whole["foff"][9]), int(whole["foff"][27]), int(whole["moff"][3]), int(whole["moff"][9])
                assert np.array_equal(part["foff"], whole["foff"][9:28] - whole["foff"][9]) and np.array_equal(part["fdoc"], whole["fdoc"][e0:e1])
                assert np.array_equal(part["moff"], whole["moff"][3:10] - whole["moff"][3]) and np.array_equal(part["mtf"], whole["mtf"][m0:m1])
        finally:
            sh.close()
    ix.close()
    return out


@pytest.mark.parametrize("positions", MODES)
def test_levels_equal_what_a_commit_prepares(S, corpus, level_reads, positions):
    ix = _index_bin(S, corpus.file)
    order = corpus.lists_of(ix)
    ix.close()
    sh = S.Shard(0)
    try:
        for level in range(3):
            hi = min(N_FILE, (level + 1) * LV)
            want = _expected_level(order, corpus.doclen, level, hi, F3, bool(positions))
            _same_level(level_reads[positions][level], want, ("against mf_level_prepare", level))
            o, d, f, t, np_, p = _csr(order, level * LV, hi)
            sh.commit_level_fields(level, corpus.doclen[:, level * LV:hi], BOOST, o, d, f, t, p if positions else None, np_ if positions else None)
        for level in range(3):
            _same_level(level_reads[positions][level], sh.read_level_fields(level, 0, len(order)), ("against commit_level_fields", level))
    finally:
        sh.close()


def test_both_modes_leave_the_same_postings(level_reads):
    for level in range(3):
        _same_level(level_reads[False][level], level_reads["host"][level], ("mode 0 against mode 2", level), POSTINGS)
        assert level_reads[False][level]["pos"] is None and level_reads["host"][level]["pos"] is not None


@pytest.mark.parametrize("positions", MODES)
def test_life_cycle_open_recommit_commit(S, N, corpus, positions):
    ix = _index_bin(S, corpus.file)
    order = corpus.lists_of(ix)
    sh = S.Shard(0)
    try:
        sh.open_index_bin_levels_fields(ix, BOOST, positions=positions)

        def commit(level, lists, hi):
            o, d, f, t, np_, p = _csr(lists, level * LV, hi)
            sh.commit_level_fields(level, corpus.doclen[:, level * LV:hi], BOOST, o, d, f, t, p if positions else None, np_ if positions else None)

        def check(lists, n_docs, extra, what):
            fresh = S.Shard(0)
            try:
                o, d, f, t, _, p = _csr(lists, 0, n_docs, stand_in=True)
                fresh.upload_lexical_fields(n_docs, corpus.doclen[:, :n_docs], BOOST, o, d, f, t, p if positions else None)
                sets = _query_set(S, corpus, lists, positions, extra)
                _assert_same(_answers(S, N, sh, sets), _answers(S, N, fresh, sets), what)
            finally:
                fresh.close()

        commit(2, order, 3 * LV)
        assert sh.incremental_info()[0] == 3
        _same_level(sh.read_level_fields(2, 0, len(order)), _expected_level(order, corpus.doclen, 2, 3 * LV, F3, bool(positions)), "level 2 re-committed")
        check(order, 3 * LV, (), "after the re-commit of level 2")
        grown = order + [corpus.new_term]
        commit(3, grown, N_FULL)
        assert sh.incremental_info()[0] == 4
        check(grown, N_FULL, (len(order),), "after the commit of level 3")
    finally:
        sh.close(); ix.close()


# ---- refusals: one in-bounds defect each
def _find_block(data, key, level, F=F3):
    """(key head, its segment's key bodies, their end, count, pivot, compression_type_pointer) of `key` in `level`"""
    rd = lambda at, n: int.from_bytes(data[at:at + n], "little")
    pos, nseg = 4, 1 << 11
    for lv in range(level + 1):
        if lv == 0:
            pos += 2
        pos += F * LV + 16
        tbl = pos
        pos += nseg * 8
        for sg in range(nseg):
            blen, nkeys = rd(tbl + 8 * sg, 4), rd(tbl + 8 * sg + 4, 4)
            if lv == level:
                for i in range(nkeys):
                    h = pos + i * HEAD
                    if rd(h, 8) == key:
                        return h, pos + nkeys * HEAD, pos + blen, rd(h + 8, 2) + 1, rd(h + HEAD - 6, 2), rd(h + HEAD - 4, 4)
            pos += blen
    raise AssertionError("key not in level")


def _host_code(N, data, key, F=F3, longest=LONGEST):
    """what ss_ref_decode_block_fields answers for the key's block of level 0 in `data`"""
    h, body, end, cnt, pivot, ctp = _find_block(data, key, 0, F)
    buf = np.frombuffer(bytes(data[body:end]), np.uint8).copy()
    blk = N.RefBlock()
    blk.block_id, blk.compression_type_pointer, blk.posting_count_m1, blk.pointer_pivot_p_docid = 0, ctp, cnt - 1, pivot
    blk.byte_array, blk.byte_array_len = buf.ctypes.data, len(buf)
    d16, first, f8, t16 = np.zeros(65536, np.uint16), np.zeros(65537, np.uint32), np.zeros(65536 * F, np.uint8), np.zeros(65536 * F, np.uint16)
    return N.lib().ss_ref_decode_block_fields(C.byref(blk), F, longest, N.ptr(d16, N.u16p), N.ptr(first, N.u32p), N.ptr(f8, N.u8p), N.ptr(t16, N.u16p))


def _defects(corpus, N):
    """{name: (file bytes, expected code)}; every defect but the doubled key head is one the host decoder refuses with that code"""
    out = {}
    base = bytearray(corpus.file)

    def record0(d, name):
        """offset of the record of rank 0 of the term's block in level 0 (a 2-byte pointer that is not embedded), and of the pointer"""
        _, body, _, cnt, pivot, ctp = _find_block(d, corpus.names[name].key, 0)
        assert ctp >> 30 == RF.CT_ARRAY and pivot == cnt
        ptr = body + (ctp & 0x3FFFFFFF)
        p = int.from_bytes(d[ptr:ptr + 2], "little")
        assert not p & 0x8000
        return ptr - p, ptr

    def add(name, d, term, code=-1):
        assert _host_code(N, base, corpus.names[term].key) > 0 and _host_code(N, d, corpus.names[term].key) == code, name
        out[name] = (bytes(d), code)

    d = bytearray(base)
    rec, _ = record0(d, "rec_f2")
    assert d[rec] == 0xA0 | (5 << 2) | 2  # FIELD_STOP_BIT_1, the stop bit, tf 5, field 2
    d[rec] |= 1
    add("a field id >= the field count in a record", d, "rec_f2")
    d = bytearray(base)
    rec, _ = record0(d, "rec_two")
    assert d[rec] == 0x80 | (5 << 2) | 0 and d[rec + 1] == 0xC0 | (5 << 2) | 2
    d[rec], d[rec + 1] = d[rec] | 2, d[rec + 1] & ~3
    add("descending fields", d, "rec_two")
    d = bytearray(base)
    rec, _ = record0(d, "rec_f2")
    d[rec] &= ~(7 << 2)
    add("tf 0", d, "rec_f2")
    d = bytearray(base)
    _, body, _, cnt, pivot, ctp = _find_block(d, corpus.names["emb_f0"].key, 0)
    ptr = body + (ctp & 0x3FFFFFFF)
    assert pivot == cnt and d[ptr + 1] >> 2 == 0x8 << 2  # tag 0x8, field slot 0
    d[ptr + 1] |= 0x0C
    add("an embedded pointer naming a field the index does not have", d, "emb_f0")
    d = bytearray(base)
    _, ptr = record0(d, "rec_f2")
    _, body, _, _, _, ctp = _find_block(d, corpus.names["rec_f2"].key, 0)
    assert (ctp & 0x3FFFFFFF) < 0x7FFF
    d[ptr:ptr + 2] = (0x7FFF).to_bytes(2, "little")
    add("a record pointer past the key bodies", d, "rec_f2")
    d = bytearray(base)
    _, body, _, cnt, pivot, ctp = _find_block(d, corpus.names["rle_one"].key, 0)
    assert ctp >> 30 == RF.CT_RLE
    cont = body + (ctp & 0x3FFFFFFF) + 2 * pivot + 3 * (cnt - pivot)
    assert int.from_bytes(d[cont:cont + 2], "little") == 1 and int.from_bytes(d[cont + 4:cont + 6], "little") == cnt - 1
    d[cont + 4:cont + 6] = cnt.to_bytes(2, "little")
    add("a count that is not its container's", d, "rle_one")
    d = bytearray(base)
    h, _, _, _, _, ctp = _find_block(d, corpus.names["a64"].key, 0)
    d[h + HEAD - 4:h + HEAD] = (ctp & 0x3FFFFFFF).to_bytes(4, "little")
    add("a Delta container", d, "a64", -4)
    # the same key head in a second segment of the level, with a copy of the first segment's key bodies: refused on the host
    h, body, end, _, _, _ = _find_block(base, corpus.names["a63"].key, 0)
    tbl = 4 + 2 + F3 * LV + 16
    pos, seg_b = tbl + 2048 * 8, None
    for sg in range(2048):
        blen, nkeys = int.from_bytes(base[tbl + 8 * sg:tbl + 8 * sg + 4], "little"), int.from_bytes(base[tbl + 8 * sg + 4:tbl + 8 * sg + 8], "little")
        if nkeys == 0 and seg_b is None:
            seg_b = (sg, pos)
        pos += blen
    extra = bytes(base[h:h + HEAD]) + bytes(base[body:end])
    d = bytearray(base[:seg_b[1]] + extra + base[seg_b[1]:])
    d[tbl + 8 * seg_b[0]:tbl + 8 * seg_b[0] + 8] = len(extra).to_bytes(4, "little") + (1).to_bytes(4, "little")
    out["a key head in two segments of one level"] = (bytes(d), -1)
    return out


@pytest.mark.parametrize("positions", MODES)
def test_refusals_leave_the_shard_as_it_was(S, N, corpus, positions):
    ix = _index_bin(S, corpus.file)
    order = corpus.lists_of(ix)
    sh = S.Shard(0)
    try:
        sh.open_index_bin_levels_fields(ix, BOOST, positions=positions)
        sets = _query_set(S, corpus, order, positions)
        before, info = _answers(S, N, sh, sets), sh.incremental_info()[:2]

        def refused(bad, code, what, mode=positions):
            with pytest.raises(N.SeekStormHipError) as e:
                sh.open_index_bin_levels_fields(bad, BOOST if bad.indexed_field_count == 3 else None, positions=mode)
            assert e.value.code == code, (what, e.value.code)
            assert sh.incremental_info()[:2] == info, what

        defects = _defects(corpus, N)
        assert len(defects) == 8
        for name, (data, code) in defects.items():
            bad = _index_bin(S, data)
            refused(bad, code, name)
            bad.close()
        tiered = _index_bin(S, corpus.file)
        assert tiered.tier(60) < tiered.term_count
        refused(tiered, N.SS_ENOTSUP, "a tiered ix")
        tiered.close()
        refused(ix, N.SS_ENOTSUP, "mode 3", "device")
        refused(ix, N.SS_EINVAL, "an unknown mode", 4)
        rng = np.random.default_rng(3)
        one = S.IndexBin(RF.write_index_bin(20, rng.integers(1, 60, 20).astype(np.uint8), [(8 << 3, np.asarray([1, 5, 9]), np.asarray([2, 1, 3]))], rng))
        refused(one, N.SS_EINVAL, "a one-field file")
        one.close()
        _assert_same(_answers(S, N, sh, sets), before, "after the refusals")
    finally:
        sh.close(); ix.close()


# ---- 2 and 8 fields: field id slots of 1 and 3 bits
def _edge_file(F, longest, rng):
    other = [f for f in range(F) if f != longest]
    a, b = (other[0], other[1]) if len(other) > 1 else (min(other[0], longest), max(other[0], longest))
    emb2 = [[(longest, [3])], [(longest, [5000])], [(longest, [3, 5])], [(longest, [40, 50])], [(other[0], [1])], [(other[0], [1, 2])], [(other[0], [1, 3, 5])],
            [(a, [1]), (b, [2])]]
    emb3 = [[(longest, [3])], [(longest, [3, 5])], [(longest, [600, 700])], [(longest, [1, 3, 5])], [(longest, [40, 50, 60])], [(longest, [1, 3, 5, 7])],
            [(longest, [20, 22, 24, 26])], [(other[0], [9])], [(other[0], [9, 11])], [(other[0], [1, 3, 5])], [(other[0], [1, 3, 5, 7])],
            [(a, [1]), (b, [2])], [(a, [1]), (b, [2, 4])], [(a, [1, 3]), (b, [2])]]
    if F > 2:
        c3 = sorted([a, b, [f for f in range(F) if f not in (a, b)][0]])
        emb3.append([(c3[0], [1]), (c3[1], [2]), (c3[2], [3])])

    def recorded():
        fs = sorted(int(x) for x in rng.choice(F, int(rng.integers(1, min(F, 4) + 1)), replace=False))
        return [(f, RF.random_positions(rng, int(rng.integers(5, 9)), 6)) for f in fs]

    n_docs = 3000
    lists, terms = [], []
    shapes = ([emb2[i % len(emb2)] for i in range(200)],                                      # 2-byte pointers, all embedded
              [recorded() for _ in range(12)] + [emb3[i % len(emb3)] for i in range(200)],     # records past the limit, then 3-byte pointers
              [recorded() for _ in range(150)], [recorded() if i % 3 else emb2[i % len(emb2)] for i in range(120)])
    for i, postings in enumerate(shapes):
        docs = np.sort(rng.choice(n_docs, len(postings), replace=False))
        d = np.asarray([int(docs[j]) for j, p in enumerate(postings) for _ in p], np.int64)
        fl = np.asarray([f for p in postings for f, _ in p], np.int64)
        tf = np.asarray([len(ps) for p in postings for _, ps in p], np.int64)
        pos = np.asarray([x for p in postings for _, ps in p for x in ps], np.uint16)
        key = (1000 + i) << 43
        lists.append(_List(key, 0, d, fl, tf, tf, pos))
        terms.append((key, d, fl, tf, [list(ps) for p in postings for _, ps in p]))
    doclen = rng.integers(1, 120, (F, n_docs)).astype(np.uint8)
    data = RF.write_index_bin(n_docs, doclen, terms, rng, key_head_size=HEAD, positions_limit=100, n_fields=F, longest_field_id=longest)
    return data, lists, doclen, n_docs


@pytest.mark.parametrize("F,longest", [(2, 1), (8, 0), (8, 7)])
@pytest.mark.parametrize("positions", MODES)
def test_two_and_eight_fields(S, N, F, longest, positions):
    from test_ref_block_fields_cpu import _tags
    data, lists, doclen, n_docs = _edge_file(F, longest, np.random.default_rng(100 + F))
    tags = set()
    for l in lists[:2]:
        h, body, end, cnt, pivot, ctp = _find_block(data, l.key, 0, F)
        tags |= _tags(data[body:end], ctp, cnt, pivot)
    assert tags == set(range(0x8, 0x10)) | set(range(0x10, 0x17)) | set(range(0x18, 0x20)) - {0x19} | ({0x17} if F > 2 else set()), sorted(tags)
    ix = _index_bin(S, data, F)
    order = [lists[[l.key for l in lists].index(k)] for k in sorted(l.key for l in lists)]
    assert ix.term_count == 4 and [ix.term_of_key(l.key) for l in order] == [0, 1, 2, 3]
    a, b = S.Shard(0), S.Shard(0)
    try:
        a.open_index_bin_levels_fields(ix, None, positions=positions)
        b.upload_index_bin(ix, None, positions=bool(positions))
        _same_level(a.read_level_fields(0, 0, 4), _expected_level(order, doclen, 0, n_docs, F, bool(positions)), ("against mf_level_prepare", F))
        sets = [([[0], [1], [2], [3], [0, 1], [2, 3], [0, 1, 2]], qt, None, ff) for qt in (S.QueryType.Union, S.QueryType.Intersection)
                for ff in (None, [longest], [0, F - 1])]
        if positions:
            sets.append(([[2, 3], [3, 2], [0, 2]], S.QueryType.Phrase, None, None))
        _assert_same(_answers(S, N, a, sets), _answers(S, N, b, sets), ("fields", F))
    finally:
        a.close(); b.close(); ix.close()
