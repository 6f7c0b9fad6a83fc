"""index.bin opened LEVEL BY LEVEL, decoded on the device, ready to commit to (ss_bm25_open_index_bin_levels / Shard.open_index_bin_levels).

One seeded corpus of 3 * 65536 + 500 docs, built as arrays: about 40 dense terms shaped so that real levels of the file hold every
container and pointer case of tests/test_ref_block_decode_cpu.py (Arrays of 1, 2, 63, 64, 65 and 4095 postings; Rle of one run, with
single-doc runs, ending at doc 65 535 of a level, a full level of 65 536 postings; Bitmaps; pivots at 0, inside and at the count through
a lowered positions_limit; tf VINTs of 1 - 3 bytes; terms absent from a level, a term only in the last level; n-gram keys of 2 and 3
components) and about 200 rare terms.  index.bin is written from the prefix of 2 * 65536 + 1000 docs: its last level is partial.

Every combination of untiered / tiered and without positions (the device decoder) / with them:
  1. the opened shard answers a fixed query set exactly as a shard given upload_index_bin of the same file;
  2. the life cycle: level 2 re-committed with the docs up to 3 * 65536, level 3 committed with the last 500 docs and new keys -- after
     each step the answers equal those of a fresh shard given one array upload of the same prefix;
  3. files with one in-bounds defect -- the same key head in two segments of one level among them, which is refused on the host before
     anything is launched -- are refused and the shard keeps its image, levels and answers.
And an Rle container of more runs than the decode kernel's table holds at a time answers as the host decoder's image does.
A fresh array upload with positions takes tf positions per posting, which the component lists of an n-gram key do not have (the key's own
positions stand behind its first component): there the fresh shards get stand-in positions for those lists, and no phrase names them."""
import numpy as np
import pytest

from oracle import ref_format as RF

pytestmark = pytest.mark.gpu

LV = 65536
N_FULL = 3 * LV + 500
N_FILE = 2 * LV + 1000
HEAD = 23            # key head with room for three component df bytes
LIMIT = 2000         # positions_limit of the writer: 3-byte pointers inside ordinary blocks
TIER_MIN = 60        # keys with fewer postings in the file are rare
COMBOS = [(False, False), (False, True), (True, False), (True, True)]  # (tiered, positions)


@pytest.fixture(scope="module")
def S():
    import seekstorm_amd
    return seekstorm_amd


class _List:
    """one posting list = one term id: docs ascending, tf, positions per posting (npos of them: the tf, except for the component lists of
    an n-gram key -- the key's own count behind component 0, none behind the others)"""

    def __init__(self, key, comp, docs, tfs, npos, pos):
        self.key, self.comp = int(key), int(comp)
        self.docs, self.tfs, self.npos, self.pos = np.asarray(docs, np.uint32), np.asarray(tfs, np.uint16), np.asarray(npos, np.uint16), np.asarray(pos, np.uint16)
        self.pstart = np.concatenate(([0], np.cumsum(self.npos.astype(np.int64))))
        assert np.all(np.diff(self.docs.astype(np.int64)) > 0) and len(self.pos) == self.pstart[-1]

    def cut(self, lo, hi):
        i0, i1 = int(np.searchsorted(self.docs, lo)), int(np.searchsorted(self.docs, hi))
        return i0, i1


def _positions(rng, counts, max_gap=8):
    """ascending positions, counts[i] of them for posting i: first absolute, small gaps (most postings embed)"""
    counts = np.asarray(counts, np.int64)
    tot = int(counts.sum())
    gaps = rng.integers(0, max_gap, tot).astype(np.int64) + 1
    c = np.cumsum(gaps)
    starts = np.cumsum(counts) - counts
    base = np.repeat(c[starts[counts > 0]] - gaps[starts[counts > 0]], counts[counts > 0])
    return (c - base - 1).astype(np.uint16)


class _Corpus:
    def __init__(self):
        rng = np.random.default_rng(515)
        self.rng = rng
        self.doclen = rng.integers(1, 120, N_FULL).astype(np.uint8)
        self.single, self.ngram = [], []   # keys of the file; n-gram: (key, [component lists])
        self.names = {}
        used = set()

        def key(ntype=0):
            while True:
                k = (int(rng.integers(1, 1 << 60)) << 3) | ntype
                if k not in used:
                    used.add(k)
                    return k

        def at(level, local):
            return [level * LV + int(x) for x in local]

        def term(name, docs, tfs=None, pos=None):
            docs = np.asarray(sorted(docs), np.uint32)
            if tfs is None:
                tfs = np.minimum(rng.geometric(0.45, len(docs)), 6)
            tfs = np.asarray(tfs, np.uint16)
            if pos is None:
                pos = _positions(rng, tfs)
            l = _List(key(), 0, docs, tfs, tfs, pos)
            self.single.append(l)
            self.names[name] = l
            return l

        spaced = lambda n, step=3, first=1: [first + step * i for i in range(n)]
        # ---- Arrays of 1, 2, 63, 64, 65, 4095 postings in a level (their other levels make them dense)
        term("a1", at(0, [777]) + at(1, spaced(100, 50)))
        term("a2", at(0, [5, 60000]) + at(1, spaced(100, 70)))
        for n in (63, 64, 65):
            term(f"a{n}", at(0, spaced(n, 11)) + at(2, [10, 500, 999, 1200]))
        term("a4095", at(1, spaced(4095, 16)))
        term("a1_last", at(0, spaced(80, 9)) + at(2, [321]))
        # ---- Rle: one run, single-doc runs, a run ending at the level's last doc and one starting at its first, the full level
        term("rle_one", at(0, range(1000, 1300)))
        term("rle_single", at(1, [5, 9, 13] + list(range(100, 400)) + [700, 65000]))
        term("rle_end", at(0, [7] + list(range(65000, 65536))) + at(1, range(0, 50)))
        full = at(1, range(LV)) + at(2, range(1500))
        term("rle_full", full, tfs=np.ones(len(full), np.uint16), pos=(np.arange(len(full)) & 3).astype(np.uint16))
        # ---- Bitmaps
        term("bm_even", at(0, range(0, 8192, 2)))
        term("bm_bits", at(0, sorted({63, 64, 65535} | {int(x) for x in rng.choice(np.arange(0, 65535, 5), 4200, replace=False)})))
        # ---- pointers: the first record of a block beyond the limit (pivot 0); tf VINTs of 1, 2 and 3 bytes; every embedded tag
        d = at(0, spaced(70, 100))
        tfs = np.concatenate(([2100], rng.integers(1, 4, 69)))
        term("pivot0", d, tfs, np.concatenate((np.arange(2100) * 3, _positions(rng, tfs[1:]))))
        d = at(1, spaced(70, 90))
        tfs = np.concatenate(([5, 200, 17000], rng.integers(1, 7, 67)))
        term("vint", d, tfs, np.concatenate((np.arange(5) * 2, np.arange(200) * 2, np.arange(17000) * 3, _positions(rng, tfs[3:]))))
        d = at(0, spaced(90, 40)) + at(2, spaced(40, 20))
        term("tags", d, tfs=[1 + i % 4 for i in range(len(d))])
        # ---- absent from a level; only in the last level
        term("absent1", at(0, spaced(100, 31)) + at(2, spaced(30, 60)))
        term("only_last", at(2, spaced(80, 12) + spaced(100, 400, 1003)))
        # ---- ordinary lists over the whole corpus: pivots inside their blocks under the lowered limit, 3-byte embedded pointers
        for i, df in enumerate((0.001, 0.0015, 0.002, 0.003, 0.004, 0.006, 0.008, 0.012, 0.016, 0.02, 0.03, 0.05, 0.1, 0.2)):
            term(f"m{i}", rng.choice(N_FULL, int(df * N_FULL), replace=False))
        # ---- n-gram keys of 2 and 3 components (dense) and one rare bigram: component tfs of every VINT size, the key's own positions
        for name, ntype, n in (("ng2", 1, 80), ("ng3", 4, 70), ("ng2_rare", 2, 10)):
            nc = 2 if ntype <= 3 else 3
            docs = np.sort(rng.choice(N_FILE, n, replace=False)).astype(np.uint32)
            counts = rng.integers(1, 4, n).astype(np.uint16)
            ctf = np.stack([rng.choice([1, 2, 90, 300, 17000], n) for _ in range(nc)], axis=1).astype(np.uint16)
            pos = _positions(rng, counts)
            k = key(ntype)
            lists = [_List(k, c, docs, ctf[:, c], counts if c == 0 else np.zeros(n, np.uint16), pos if c == 0 else np.zeros(0, np.uint16)) for c in range(nc)]
            self.ngram.append((k, lists, counts, ctf, pos))
            self.names[name] = lists
        self.n_crafted = len(self.single)
        # ---- rare terms: 1 - 20 postings, at least one inside the file; some only in the file's last level
        for i in range(200):
            n = int(rng.integers(1, 21))
            if i % 10 == 0:
                docs = set(int(x) for x in rng.integers(2 * LV, N_FILE, min(n, 5)))
            else:
                docs = {int(rng.integers(0, N_FILE))} | set(int(x) for x in rng.integers(0, N_FULL, n - 1))
            term(f"r{i}", docs)
        # ---- keys that only the last commit brings: two rare ones, one frequent one (the untiered run)
        self.new_rare = [_List(key(), 0, d, t, t, _positions(rng, t)) for d, t in
                         ((np.asarray([3 * LV + 3, 3 * LV + 77, 3 * LV + 499], np.uint32), np.asarray([1, 3, 2], np.uint16)),
                          (np.asarray([3 * LV], np.uint32), np.asarray([4], np.uint16)))]
        d = np.asarray(at(3, spaced(150, 3)), np.uint32)
        t = np.minimum(rng.geometric(0.45, len(d)), 6).astype(np.uint16)
        self.new_dense = _List(key(), 0, d, t, t, _positions(rng, t))
        self.file = self._write()

    def _write(self):
        def per_posting(l, i1):
            return [[int(x) for x in l.pos[l.pstart[i]:l.pstart[i + 1]]] for i in range(i1)]
        terms, ngram_terms = [], []
        for l in self.single:
            _, i1 = l.cut(0, N_FILE)
            assert i1 > 0
            terms.append((l.key, l.docs[:i1].astype(np.int64), l.tfs[:i1], per_posting(l, i1)))
        for k, lists, counts, ctf, pos in self.ngram:
            ngram_terms.append((k, lists[0].docs.astype(np.int64), counts, ctf, [40 + c for c in range(len(lists))], per_posting(lists[0], len(counts))))
        return RF.write_index_bin(N_FILE, self.doclen[:N_FILE], terms, self.rng, key_head_size=HEAD, positions_limit=LIMIT, ngram_terms=ngram_terms)

    def lists_of(self, ix, tiered):
        """the file's lists in term-id order, the dense count"""
        every = list(self.single) + [l for _, lists, *_ in self.ngram for l in lists]
        ids = {}
        for l in every:
            t = ix.term_of_key(l.key)
            assert t is not None
            ids[t + l.comp] = l
        assert sorted(ids) == list(range(ix.term_count))
        return [ids[t] for t in range(ix.term_count)], (ix.n_dense if tiered else ix.term_count)

    def term_id(self, order, name):
        l = self.names[name]
        return tuple(order.index(x) for x in l) if isinstance(l, list) else order.index(l)


def _csr(lists, lo, hi, stand_in=False):
    """CSR over the lists of their postings with lo <= doc < hi: (offs, docs, tfs, npos, positions); stand_in: tf ascending stand-in
    positions where a list's postings do not carry tf positions (n-gram component lists, for uploads that take tf positions each)"""
    offs, docs, tfs, npos, pos = [0], [], [], [], []
    for l in lists:
        i0, i1 = l.cut(lo, hi)
        offs.append(offs[-1] + i1 - i0)
        docs.append(l.docs[i0:i1]); tfs.append(l.tfs[i0:i1])
        if stand_in and not np.array_equal(l.npos, l.tfs):
            t = l.tfs[i0:i1].astype(np.int64)
            npos.append(l.tfs[i0:i1])
            pos.append((np.arange(int(t.sum())) - np.repeat(np.cumsum(t) - t, t)).astype(np.uint16))
        else:
            npos.append(l.npos[i0:i1]); pos.append(l.pos[l.pstart[i0]:l.pstart[i1]])
    cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dt)
    return np.asarray(offs, np.uint64), cat(docs, np.uint32), cat(tfs, np.uint16), cat(npos, np.uint16), cat(pos, np.uint16)


@pytest.fixture(scope="module")
def corpus():
    return _Corpus()


def _index_bin(S, corpus, tiered, data=None):
    ix = S.IndexBin(corpus.file if data is None else data, key_head_size=HEAD)
    if tiered:
        ix.tier(TIER_MIN)
    return ix


def _fresh(S, corpus, lists, nd, n_docs, positions):
    """a shard given ONE array upload of the prefix of n_docs docs: the dense lists, and the others appended as whole sparse lists"""
    sh = S.Shard(0)
    o, d, t, _, p = _csr(lists[:nd], 0, n_docs, stand_in=True)
    sh.upload_lexical(n_docs, corpus.doclen[:n_docs], o, d, t, p if positions else None)
    if nd < len(lists):
        o, d, t, np_, p = _csr(lists[nd:], 0, n_docs)
        assert sh.append_sparse(o, d, t, p if positions else None, np_ if positions else None) == nd
    return sh


def _query_set(S, corpus, order, nd, positions, extra=()):
    """[(term lists, query type, not lists)]: single terms of every crafted shape, 2-term ANDs, 3-term ORs, queries naming rare terms and
    NOT terms; phrases where positions were opened"""
    T = lambda name: corpus.term_id(order, name)
    crafted = [order.index(l) for l in corpus.single[:corpus.n_crafted]]
    rare = [order.index(corpus.names[f"r{i}"]) for i in (0, 3, 10, 17, 50, 120, 199)] + list(extra)
    m = [T(f"m{i}") for i in range(14)]
    sets = []
    singles = [[t] for t in crafted + rare] + [[T("ng2")], [T("ng3")], [T("ng2_rare")]]
    sets.append((singles, S.QueryType.Union, None))
    ands = [[m[13], m[12]], [m[11], m[10]], [m[9], m[11]], [m[8], m[3]], [T("rle_full"), m[11]], [T("bm_even"), m[10]], [T("bm_bits"), T("rle_end")],
            [T("a4095"), T("rle_full")], [T("tags"), m[11]], [T("only_last"), T("rle_full")], [T("absent1"), T("a63")], [m[11], rare[0]],
            [T("rle_full"), rare[3]], [rare[1], rare[2]], [T("ng2"), m[11]], [m[10], T("ng3")], [T("vint"), T("rle_full")]]
    sets.append((ands, S.QueryType.Intersection, None))
    ors = [[m[13], m[12], m[11]], [m[11], m[10], m[9]], [m[0], m[1], m[2]], [T("a1"), T("a2"), T("a63")], [T("pivot0"), T("vint"), T("tags")], [m[5], rare[0], rare[4]],
           [rare[1], rare[2], rare[5]], [T("rle_one"), T("rle_single"), T("bm_even")], [T("only_last"), T("a1_last"), rare[6]],
           [T("ng2"), m[4], m[6]], [T("ng2_rare"), m[7], T("absent1")]]
    sets.append((ors, S.QueryType.Union, None))
    nots = [([m[11], m[10]], [m[9]]), ([m[11]], [T("rle_full")]), ([T("bm_even"), m[8]], [m[11], m[10]]), ([m[9], rare[0]], [m[11]]),
            ([m[10]], [rare[4]]), ([T("rle_full")], [T("bm_bits"), m[11]])]
    sets.append(([a for a, _ in nots], S.QueryType.Union, [b for _, b in nots]))
    sets.append(([a for a, _ in nots[:3]], S.QueryType.Intersection, [b for _, b in nots[:3]]))
    if positions:
        phrases = [[m[13], m[12]], [m[11], m[10]], [m[10], m[11]], [T("rle_full"), m[11]], [m[11], T("rle_full")], [m[9], m[11], m[10]], [T("tags"), m[11]],
                   [m[11], rare[0]], [rare[4], m[11]], [T("bm_even"), T("bm_bits")], [T("rle_full"), T("rle_full")]]
        sets.append((phrases, S.QueryType.Phrase, None))
    return sets


def _answers(S, sh, sets):
    out = []
    for terms, qt, nots in sets:
        q = sh.make_queries(terms, qt, nots)
        for k, rt in ((10, S.ResultType.TopkCount), (100, S.ResultType.TopkCount), (10, S.ResultType.Count)):
            out.append(sh.search_lexical_batch(q, k, rt))
    return out


def _assert_same(a, b, what):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        for u, v, name in zip(x, y, ("doc", "score", "count", "total")):
            u, v = (u.view(np.uint32), v.view(np.uint32)) if name == "score" else (u, v)
            assert np.array_equal(u, v), (what, i, name, np.argwhere(u != v)[:4].tolist())


@pytest.mark.parametrize("tiered,positions", COMBOS)
def test_opened_levels_answer_as_the_uploaded_file(S, corpus, tiered, positions):
    ix = _index_bin(S, corpus, tiered)
    assert ix.level_count == 3 and ix.indexed_doc_count == N_FILE
    order, nd = corpus.lists_of(ix, tiered)
    assert (nd < len(order)) == tiered and nd >= corpus.n_crafted
    a, b = S.Shard(0), S.Shard(0)
    try:
        a.open_index_bin_levels(ix, positions=positions)
        b.upload_index_bin(ix, positions=positions)
        assert a.incremental_info()[0] == 3 and b.incremental_info()[0] == 0
        sets = _query_set(S, corpus, order, nd, positions)
        got, want = _answers(S, a, sets), _answers(S, b, sets)
        _assert_same(got, want, "open_index_bin_levels against upload_index_bin")
        assert all(int(x[3].min()) > 0 for x in want[:3])  # (every single term is found)
        if positions:
            assert sum(int(x[3].sum()) for x in want[-3:]) > 0  # (some phrase matches)
    finally:
        a.close(); b.close(); ix.close()


@pytest.mark.parametrize("tiered,positions", COMBOS)
def test_life_cycle_open_recommit_commit(S, corpus, tiered, positions):
    ix = _index_bin(S, corpus, tiered)
    order, nd = corpus.lists_of(ix, tiered)
    sh = S.Shard(0)
    try:
        sh.open_index_bin_levels(ix, positions=positions)

        def commit(level, lists, hi):
            o, d, t, np_, p = _csr(lists, level * LV, hi)
            sh.commit_level(level, corpus.doclen[level * LV:hi], o, d, t, nd if tiered else None, p if positions else None, np_ if positions else None)

        def check(lists, n_docs, extra, what):
            fresh = _fresh(S, corpus, lists, nd if tiered else len(lists), n_docs, positions)
            try:
                sets = _query_set(S, corpus, lists, nd, positions, extra)
                _assert_same(_answers(S, sh, sets), _answers(S, fresh, sets), what)
            finally:
                fresh.close()

        # the file's last level was incomplete: it is committed again, now full
        commit(2, order, 3 * LV)
        assert sh.incremental_info()[0] == 3
        check(order, 3 * LV, (), "after the re-commit of level 2")
        # the next level, with keys the file did not hold: they take the next ids (a frequent one only where every term is dense)
        grown = order + ([] if tiered else [corpus.new_dense]) + corpus.new_rare
        commit(3, grown, N_FULL)
        assert sh.incremental_info()[0] == 4
        check(grown, N_FULL, tuple(range(len(order), len(grown))), "after the commit of level 3")
    finally:
        sh.close(); ix.close()


# ---- refusals: one in-bounds defect each
def _find_block(data, key, level):
    """(offset of the key head, offset of its segment's key bodies, count, pivot, compression_type_pointer) of `key` in `level`"""
    rd = lambda at, n: int.from_bytes(data[at:at + n], "little")
    pos, nseg = 4, 1 << 11
    for lv in range(level + 1):
        if lv == 0:
            pos += 2
        pos += LV + 16
        tbl = pos
        pos += nseg * 8
        for sg in range(nseg):
            blen, nkeys = rd(tbl + 8 * sg, 4), rd(tbl + 8 * sg + 4, 4)
            if lv == level:
                for i in range(nkeys):
                    h = pos + i * HEAD
                    if rd(h, 8) == key:
                        return h, pos + nkeys * HEAD, rd(h + 8, 2) + 1, rd(h + HEAD - 6, 2), rd(h + HEAD - 4, 4)
            pos += blen
    raise AssertionError("key not in level")


def _defects(corpus):
    """{name: (file bytes, expected code)}"""
    out = {}
    base = bytearray(corpus.file)
    # an Array with two docs swapped
    d = bytearray(base)
    _, body, cnt, pivot, ctp = _find_block(d, corpus.names["a63"].key, 0)
    assert ctp >> 30 == RF.CT_ARRAY and pivot == cnt
    cont = body + (ctp & 0x3FFFFFFF) + 2 * cnt
    d[cont:cont + 2], d[cont + 2:cont + 4] = d[cont + 2:cont + 4], d[cont:cont + 2]
    out["array docs swapped"] = (bytes(d), -1)
    # a record's count VINT of 0 (two bytes, as the 2100 it replaces)
    d = bytearray(base)
    _, body, cnt, pivot, ctp = _find_block(d, corpus.names["pivot0"].key, 0)
    assert pivot == 0
    rng_ = body + (ctp & 0x3FFFFFFF)
    back = int.from_bytes(d[rng_:rng_ + 3], "little")
    assert back < 0x800000 and bytes(d[rng_ - back:rng_ - back + 2]) == RF.vint(2100)
    d[rng_ - back:rng_ - back + 2] = bytes([0x00, 0x80])
    out["record count 0"] = (bytes(d), -1)
    # an Rle run one doc longer than the key head's count
    d = bytearray(base)
    _, body, cnt, pivot, ctp = _find_block(d, corpus.names["rle_one"].key, 0)
    assert ctp >> 30 == RF.CT_RLE
    cont = body + (ctp & 0x3FFFFFFF) + 2 * pivot + 3 * (cnt - pivot)
    assert int.from_bytes(d[cont:cont + 2], "little") == 1 and int.from_bytes(d[cont + 4:cont + 6], "little") == cnt - 1
    d[cont + 4:cont + 6] = cnt.to_bytes(2, "little")
    out["rle run sum off by one"] = (bytes(d), -1)
    # the same key head in a second segment of the level (an empty one gets the head and a copy of the first segment's key bodies, so the
    # head's pointers stay inside the bodies): two blocks of one key in one level.  Refused on the host, before anything is launched
    k = corpus.names["a63"].key
    h, body, _, _, _ = _find_block(base, k, 0)
    tbl = 4 + 2 + LV + 16
    pos, seg_a, seg_b = tbl + 2048 * 8, None, None
    for sg in range(2048):
        blen, nkeys = int.from_bytes(base[tbl + 8 * sg:tbl + 8 * sg + 4], "little"), int.from_bytes(base[tbl + 8 * sg + 4:tbl + 8 * sg + 8], "little")
        if pos <= h < pos + blen:
            seg_a = (pos + nkeys * HEAD, pos + blen)
        elif nkeys == 0 and seg_b is None:
            seg_b = (sg, pos)
        pos += blen
    extra = bytes(base[h:h + HEAD]) + bytes(base[seg_a[0]:seg_a[1]])
    d = bytearray(base[:seg_b[1]] + extra + base[seg_b[1]:])
    d[tbl + 8 * seg_b[0]:tbl + 8 * seg_b[0] + 8] = len(extra).to_bytes(4, "little") + (1).to_bytes(4, "little")
    out["key head in two segments of a level"] = (bytes(d), -1)
    # container type Delta
    d = bytearray(base)
    h, _, _, _, ctp = _find_block(d, corpus.names["a64"].key, 0)
    d[h + HEAD - 4:h + HEAD] = (ctp & 0x3FFFFFFF).to_bytes(4, "little")
    out["delta container"] = (bytes(d), -4)
    return out


@pytest.mark.parametrize("positions", [False, True])
def test_defective_files_are_refused_and_the_shard_keeps_its_image(S, corpus, positions):
    from seekstorm_amd import _native as N
    ix = _index_bin(S, corpus, True)
    order, nd = corpus.lists_of(ix, True)
    sh = S.Shard(0)
    try:
        sh.open_index_bin_levels(ix, positions=positions)
        sets = _query_set(S, corpus, order, nd, positions)
        before, info = _answers(S, sh, sets), sh.incremental_info()[:2]
        for name, (data, code) in _defects(corpus).items():
            for tiered in (False, True):
                bad = _index_bin(S, corpus, tiered, data)
                with pytest.raises(N.SeekStormHipError) as e:
                    sh.open_index_bin_levels(bad, positions=positions)
                bad.close()
                assert e.value.code == code, (name, tiered, e.value.code)
                assert sh.incremental_info()[:2] == info, name
        # an index of several indexed fields: not this entry's
        rng = np.random.default_rng(3)
        docs, fields, tfs = np.asarray([1, 1, 5, 9]), np.asarray([0, 2, 1, 2]), np.asarray([2, 1, 3, 1])
        three = S.IndexBin(RF.write_index_bin(20, rng.integers(1, 60, (3, 20)).astype(np.uint8), [(8 << 3, docs, fields, tfs)], rng, n_fields=3,
                                              longest_field_id=1), indexed_field_count=3)
        with pytest.raises(N.SeekStormHipError) as e:
            sh.open_index_bin_levels(three, positions=positions)
        three.close()
        assert e.value.code == N.SS_ENOTSUP and sh.incremental_info()[:2] == info
        _assert_same(_answers(S, sh, sets), before, "after the refusals")
    finally:
        sh.close(); ix.close()



def test_rle_container_of_more_runs_than_one_round(S, monkeypatch):
    """an Rle container of 3000 runs -- larger than the Bitmap the writer would choose, so the writer's chooser is overridden for that one
    list -- is decoded by the device path in two rounds of its run table and answers as the host decoder's image does"""
    rng = np.random.default_rng(9)
    n_docs = LV
    long_docs = np.asarray([20 * i + j for i in range(3000) for j in (0, 1)], np.int64)
    chooser = RF.container

    def forced(local_docs):
        d = np.asarray(local_docs, np.int64)
        if len(d) == len(long_docs) and np.array_equal(d, long_docs):
            out = bytearray((3000).to_bytes(2, "little"))
            for i in range(3000):
                out += int(20 * i).to_bytes(2, "little") + (1).to_bytes(2, "little")
            return RF.CT_RLE, bytes(out)
        return chooser(local_docs)
    monkeypatch.setattr(RF, "container", forced)
    other = np.sort(rng.choice(n_docs, 5000, replace=False)).astype(np.int64)
    tf = lambda n: np.minimum(rng.geometric(0.45, n), 6).astype(np.uint16)
    data = RF.write_index_bin(n_docs, rng.integers(1, 120, n_docs).astype(np.uint8), [(1 << 3, long_docs, tf(len(long_docs))), (2 << 3, other, tf(5000))],
                              rng, key_head_size=HEAD, positions_limit=LIMIT)
    ix = S.IndexBin(data, key_head_size=HEAD)
    from seekstorm_amd import _native as N
    h, body, cnt, pivot, ctp = _find_block(data, 1 << 3, 0)
    assert ctp >> 30 == RF.CT_RLE and cnt == 6000
    a, b = S.Shard(0), S.Shard(0)
    try:
        a.open_index_bin_levels(ix)
        b.upload_index_bin(ix)
        sets = [([[0], [1], [0, 1]], S.QueryType.Union, None), ([[0, 1]], S.QueryType.Intersection, None)]
        _assert_same(_answers(S, a, sets), _answers(S, b, sets), "a long Rle container")
        assert int(_answers(S, a, sets)[2][3][0]) == 6000
    finally:
        a.close(); b.close(); ix.close()
