"""index.bin opened level by level WITH POSITIONS decoded on the device (ss_bm25_open_index_bin_levels mode SS_OPEN_POSITIONS_DEVICE /
Shard.open_index_bin_levels(ix, positions="device")), and the read-backs of what an open or a commit left in HBM
(Shard.open_info / read_level / read_sparse).

One seeded corpus whose file holds 65536 + 300 docs in two levels, the last one partial -- the smallest shape with a level seam, rare
lists spanning levels and last-level accounting --, written with a lowered positions_limit so that 2- and 3-byte pointers, embedded and
recorded, meet inside ordinary blocks.  Terms: the position cases of tests/test_ref_block_positions_cpu.py (stored values at the
1 -> 2 -> 3-byte seams, first positions of 16384 and 65535, a running position of exactly 65535, postings of 63 / 64 / 65 / 17000
positions, 2- and 3-byte values across a 64-byte chunk boundary) in both levels and in a rare list; a term absent from level 1 and one
only in level 1; n-gram keys of 2 and 3 components (their component lists hold postings but no positions); a Bitmap, an Rle and a
full-level Rle block of 65536 postings; lists of 255 / 256 / 257 postings; about 50 rare terms, some only in the last level.  The corpus
is checked against the host decoder's postings and positions of the file while it is built.

  1. what the device left in HBM: after mode 3, untiered and tiered, open_info says the device ran, and read_level of every level and
     read_sparse of the tier equal the corpus's lists exactly -- and the read-backs of a shard opened in mode 2, bit for bit;
  2. answers: singles, ANDs, ORs, NOTs and phrases (rare terms, n-gram keys, the long postings) answer as after
     upload_index_bin(positions=True), and through the life cycle -- the partial level committed again, a further level with new keys
     -- as a fresh array upload; after the re-commit read_sparse equals the corpus's prefix;
  3. refusals, one defect per file: a gap that takes a position to 65536 (SS_ENOTSUP); a record whose positions run past
     byte_array_len, a count VINT of 0, a pointer reaching back beyond the pointer range, twenty pointers of a block redirected to its
     17000-position record (SS_EINVAL each) -- the code mode 2 gives, in both tiers, and the shard keeps its image, levels and answers;
  4. a mode outside 0..3 is SS_EINVAL and changes nothing."""
import numpy as np
import pytest

from oracle import ref_format as RF
from test_gpu_open_levels import HEAD, LIMIT, LV, TIER_MIN, _List, _answers, _assert_same, _csr, _find_block, _fresh, _positions

pytestmark = pytest.mark.gpu

N_FILE = LV + 300          # the file: level 1 is partial
N_FULL = 2 * LV + 200      # the corpus: level 1 complete, 200 docs of level 2


@pytest.fixture(scope="module")
def S():
    import seekstorm_amd
    return seekstorm_amd


def _from_stored(stored):
    """absolute positions of the stored values: the first as it is, then previous + stored + 1"""
    out = []
    for i, v in enumerate(stored):
        out.append(v if i == 0 else out[-1] + v + 1)
    return out


def _position_cases(rng):
    """[positions of one posting]: the cases of the CPU test that a whole index can hold"""
    out = []
    for v in (127, 128, 16383, 16384):
        out += [_from_stored([v, 1, v, 0, 2]), _from_stored([5, v, v])]
    out += [[16384, 16390, 20000], [16384], [65535], [3, 65535], _from_stored([60000, 5000, 533])]
    for n in (63, 64, 65):
        out += [list(range(0, 3 * n, 3)), RF.random_positions(rng, n, 300)]
    out.append(_from_stored([int(x) for x in rng.choice([0, 1, 100, 127, 128, 129, 300], 170)] + [16384, 3, 16383, 0]))
    for lead in (61, 62, 63, 64, 65):
        out.append(_from_stored([1] * lead + [16384 + lead, 200, 2, 16500] + [3] * 70))
        out.append(_from_stored([0] * lead + [128 + lead, 16384, 1] + [130] * 70))
    assert all(p[-1] <= 65535 and all(b > a for a, b in zip(p, p[1:])) for p in out)
    return out


class _Corpus:
    def __init__(self):
        rng = np.random.default_rng(616)
        self.rng = rng
        self.doclen = rng.integers(1, 120, N_FULL).astype(np.uint8)
        self.single, self.ngram, self.names = [], [], {}
        used, segs = set(), set()

        def key(ntype=0, own_segment=False):
            while True:
                k = (int(rng.integers(1, 1 << 60)) << 3) | ntype
                if k not in used and not (own_segment and ((k >> 40) & 2047) in segs):
                    used.add(k)
                    return k

        def term(name, docs, per_posting=None, tfs=None, k=None):
            """per_posting: {index of the posting: its positions}; the others draw small tfs and gaps"""
            docs = np.asarray(sorted(docs), np.uint32)
            if tfs is None:
                tfs = np.minimum(rng.geometric(0.45, len(docs)), 6)
            tfs = np.asarray(tfs, np.int64).copy()
            for i, p in (per_posting or {}).items():
                tfs[i] = len(p)
            pos = _positions(rng, tfs)
            start = np.cumsum(tfs) - tfs
            for i, p in (per_posting or {}).items():
                pos[start[i]:start[i] + len(p)] = p
            l = _List(key() if k is None else k, 0, docs, tfs, tfs, pos)
            self.single.append(l)
            self.names[name] = l
            return l

        spaced = lambda n, step=3, first=1: [first + step * i for i in range(n)]
        at = lambda level, local: [level * LV + int(x) for x in local]
        cases = _position_cases(rng)
        self.n_cases = len(cases)
        # ---- the position cases in level 0, in the partial level 1 (behind ordinary postings), and spread over a rare list of both levels
        term("pcases0", at(0, spaced(len(cases) + 40, 11)), {i: p for i, p in enumerate(cases)})
        term("pcases1", at(0, spaced(45, 13)) + at(1, spaced(len(cases), 7)), {45 + i: p for i, p in enumerate(cases)})
        rare_cases = [cases[i] for i in (0, 7, 10, 12, 15, 17, 18, 20)] + [list(range(0, 51000, 3))]
        term("rare_long", at(0, spaced(5, 900)) + at(1, spaced(4, 31)) + at(2, [5]), {i: p for i, p in enumerate(rare_cases)})
        # ---- 17000 positions in front of its block (every pointer of the block is 3-byte); the defect files redirect pointers to it
        term("big", at(0, spaced(70, 100)), {0: list(range(0, 51000, 3)), 1: list(range(0, 400, 2))})
        # ---- a body alone in its segment whose only record is followed by quiet bytes: single positions of 0, an Rle container from doc 0
        # (a count grown to 16383 runs over them past byte_array_len before any position passes 65535)
        self.tail_record = list(range(130))
        # (the key is drawn last: its segment must hold no other key)
        # ---- absent from level 1; only in level 1
        term("absent1", at(0, spaced(100, 31)) + at(2, spaced(30, 6)))
        term("only1", at(1, spaced(80, 3) + [290, 299]) + at(1, spaced(60, 500, 1003)))
        # ---- containers: Bitmap, Rle, the full level (65 536 postings cross every tile of the scan), Arrays of 255 / 256 / 257 postings
        term("bm_even", at(0, range(0, 8192, 2)))
        term("rle_one", at(0, range(1000, 1300)) + at(1, range(100, 180)))
        full = at(0, range(LV)) + at(1, range(LV))
        term("rle_full", full, tfs=np.ones(len(full), np.uint16))
        for n in (255, 256, 257):
            term(f"a{n}", at(0, spaced(n, 17)) + at(1, spaced(20, 13)))
        # ---- ordinary lists over the whole corpus
        for i, df in enumerate((0.004, 0.008, 0.02, 0.05, 0.1, 0.2)):
            term(f"m{i}", rng.choice(N_FULL, int(df * N_FULL), replace=False))
        # ---- n-gram keys of 2 and 3 components (dense) and one rare bigram: the key's own positions behind its first component
        for name, ntype, n in (("ng2", 1, 90), ("ng3", 4, 80), ("ng2_rare", 2, 12)):
            nc = 2 if ntype <= 3 else 3
            docs = np.sort(rng.choice(N_FILE, n, replace=False)).astype(np.uint32)
            counts = rng.choice([1, 2, 3, 65, 70], n).astype(np.uint16)
            ctf = np.stack([rng.choice([1, 2, 90, 300, 17000], n) for _ in range(nc)], axis=1).astype(np.uint16)
            pos = _positions(rng, counts)
            k = key(ntype)
            lists = [_List(k, c, docs, ctf[:, c], counts if c == 0 else np.zeros(n, np.uint16), pos if c == 0 else np.zeros(0, np.uint16)) for c in range(nc)]
            self.ngram.append((k, lists, counts, ctf, pos))
            self.names[name] = lists
        self.n_crafted = len(self.single)
        # ---- about 50 rare terms: 1 - 20 postings, at least one inside the file; some only in the file's last level
        for i in range(50):
            n = int(rng.integers(1, 21))
            if i % 8 == 0:
                docs = set(int(x) for x in rng.integers(LV, N_FILE, min(n, 5)))
            else:
                docs = {int(rng.integers(0, N_FILE))} | set(int(x) for x in rng.integers(0, N_FULL, n - 1))
            term(f"r{i}", docs)
        segs.update((l.key >> 40) & 2047 for l in self.single)
        segs.update((k >> 40) & 2047 for k, *_ in self.ngram)
        term("tail", at(0, range(0, 70)), {0: self.tail_record, **{i: [0] for i in range(1, 70)}}, k=key(own_segment=True))
        # ---- keys that only the last commit brings
        self.new_rare = [_List(key(), 0, d, t, t, _positions(rng, t)) for d, t in
                         ((np.asarray([2 * LV + 3, 2 * LV + 77, 2 * LV + 199], np.uint32), np.asarray([1, 3, 2], np.uint16)),
                          (np.asarray([2 * LV], np.uint32), np.asarray([4], np.uint16)))]
        d = np.asarray(at(2, spaced(60, 3)), np.uint32)
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


@pytest.fixture(scope="module")
def corpus(S):
    c = _Corpus()
    # the corpus against the host decoder's reading of the file it wrote: postings, counts and positions of every list
    ix = S.IndexBin(c.file, key_head_size=HEAD)
    try:
        assert ix.level_count == 2 and ix.indexed_doc_count == N_FILE
        order, _ = c.lists_of(ix, False)
        got, want = ix.decode_all(positions=True), _csr(order, 0, N_FILE)
        for g, w, name in zip(got, want, ("offs", "docs", "tfs", "npos", "positions")):
            assert np.array_equal(g, w), name
        # every case is there: records of more than 64 positions in both levels and in a rare list, component lists without positions
        for name, n_long in (("pcases0", 13), ("pcases1", 13), ("rare_long", 4)):
            assert np.count_nonzero(c.names[name].npos > 64) >= n_long, name
        assert int(c.names["rare_long"].npos.max()) == 17000 and int(c.names["big"].npos.max()) == 17000
        assert all(int(l.npos.sum()) == 0 for l in c.names["ng3"][1:]) and int(c.names["ng3"][0].npos.sum()) > 0
        assert c.names["rle_full"].cut(0, LV) == (0, LV)
    finally:
        ix.close()
    return c


def _index_bin(S, corpus, tiered, data=None):
    ix = S.IndexBin(corpus.file if data is None else data, key_head_size=HEAD)
    if tiered:
        ix.tier(TIER_MIN)
    return ix


def _read_all(sh, n_levels, nd, n_lists):
    """every level's arrays over the dense terms, and the tier's over its lists"""
    out = [sh.read_level(l, 0, nd) for l in range(n_levels)]
    if n_lists > nd:
        out.append(sh.read_sparse(0, n_lists - nd))
    return out


def _assert_read(got, want, what):
    for g, w, name in zip(got, want, ("offs", "docs", "tfs", "npos", "positions")):
        assert g.dtype == w.dtype and np.array_equal(g, w), (what, name, len(g), len(w), np.argwhere(g[:min(len(g), len(w))] != w[:min(len(g), len(w))])[:4].tolist())


@pytest.mark.parametrize("tiered", [False, True])
def test_device_left_the_corpus_in_hbm(S, corpus, tiered):
    ix = _index_bin(S, corpus, tiered)
    order, nd = corpus.lists_of(ix, tiered)
    assert (nd < len(order)) == tiered
    if tiered:  # the crafted dense terms stay dense, the long rare list is rare
        assert order.index(corpus.names["rare_long"]) >= nd and order.index(corpus.names["ng2_rare"][0]) >= nd
        assert all(order.index(corpus.names[n]) < nd for n in ("pcases0", "pcases1", "big", "tail", "only1", "absent1", "rle_full"))
    a, b = S.Shard(0), S.Shard(0)
    try:
        a.open_index_bin_levels(ix, positions="device")
        b.open_index_bin_levels(ix, positions="host")
        mode, post_dev, pos_dev, pos_host = a.open_info()
        all_post = sum(l.cut(0, N_FILE)[1] for l in order)
        all_pos = sum(int(l.npos[:l.cut(0, N_FILE)[1]].astype(np.int64).sum()) for l in order)
        assert (mode, post_dev, pos_dev, pos_host) == (3, all_post, all_pos, 0)
        assert b.open_info() == (2, 0, 0, all_pos)
        assert a.incremental_info()[0] == 2
        got, same = _read_all(a, 2, nd, len(order)), _read_all(b, 2, nd, len(order))
        for l in range(2):
            want = _csr(order[:nd], l * LV, min((l + 1) * LV, N_FILE))
            _assert_read(got[l], want, f"level {l} against the corpus")
            # the component lists of the n-gram keys hold postings and no positions
            t = corpus.term_id(order, "ng3")[1]
            assert got[l][0][t + 1] >= got[l][0][t] and int(got[l][3][int(got[l][0][t]):int(got[l][0][t + 1])].sum()) == 0
        if tiered:
            _assert_read(got[2], _csr(order[nd:], 0, N_FILE), "the tier against the corpus")
        for i, (g, w) in enumerate(zip(got, same)):
            _assert_read(g, w, f"read-back {i}: mode 3 against mode 2")
        # a slice of terms, sizes only, a cap too small
        t0 = corpus.term_id(order, "pcases1")
        o, d, t, n, p = a.read_level(1, t0, t0 + 1)
        w = _csr([corpus.names["pcases1"]], LV, N_FILE)
        _assert_read((o, d, t, n, p), w, "one term of level 1")
    finally:
        a.close(); b.close(); ix.close()


def _query_set(S, corpus, order, ngram_phrases, extra=()):
    T = lambda name: corpus.term_id(order, name)
    crafted = [order.index(l) for l in corpus.single[:corpus.n_crafted]] + [T("tail")]
    rare = [order.index(corpus.names[f"r{i}"]) for i in (0, 3, 8, 17, 24, 40, 49)] + [T("rare_long")] + list(extra)
    m = [T(f"m{i}") for i in range(6)]
    sets = [([[t] for t in crafted + rare] + [[T("ng2")], [T("ng3")], [T("ng2_rare")]], S.QueryType.Union, None)]
    ands = [[m[5], m[4]], [m[3], m[2]], [T("rle_full"), m[3]], [T("bm_even"), m[4]], [T("pcases0"), T("rle_full")], [T("pcases1"), m[5]], [T("only1"), T("rle_full")],
            [T("absent1"), T("a255")], [m[5], rare[0]], [T("rle_full"), T("rare_long")], [rare[1], rare[2]], [T("ng2"), m[5]], [T("big"), T("rle_full")]]
    sets.append((ands, S.QueryType.Intersection, None))
    ors = [[m[5], m[4], m[3]], [m[0], m[1], m[2]], [T("a255"), T("a256"), T("a257")], [T("pcases0"), T("big"), T("tail")], [m[3], rare[0], T("rare_long")],
           [T("rle_one"), T("bm_even"), T("only1")], [T("ng2"), m[2], m[4]], [T("ng2_rare"), m[1], T("absent1")]]
    sets.append((ors, S.QueryType.Union, None))
    nots = [([m[5], m[4]], [m[3]]), ([m[5]], [T("rle_one")]), ([m[3], rare[0]], [m[5]]), ([m[4]], [T("rare_long")]), ([T("rle_full")], [T("bm_even"), m[5]])]
    sets.append(([a for a, _ in nots], S.QueryType.Union, [b for _, b in nots]))
    phrases = [[m[5], m[4]], [m[4], m[5]], [T("rle_full"), m[5]], [m[5], T("rle_full")], [m[3], m[5], m[4]], [m[5], rare[0]], [T("rare_long"), m[5]],
               [T("rare_long"), T("rle_full")], [T("pcases0"), T("rle_full")], [T("rle_full"), T("pcases1")], [T("big"), T("tail")], [T("tail"), T("big")],
               [T("pcases0"), T("pcases1")], [T("big"), T("rle_full")], [T("rle_full"), T("rle_full")]]
    if ngram_phrases:
        phrases += [[T("ng2"), m[5]], [m[5], T("ng3")], [T("ng2"), T("rle_full")], [T("rle_full"), T("ng3")], [T("ng2_rare"), T("rle_full")], [T("ng2"), T("ng3")]]
    sets.append((phrases, S.QueryType.Phrase, None))
    return sets


@pytest.mark.parametrize("tiered", [False, True])
def test_answers_and_life_cycle(S, corpus, tiered):
    ix = _index_bin(S, corpus, tiered)
    order, nd = corpus.lists_of(ix, tiered)
    sh, up = S.Shard(0), S.Shard(0)
    try:
        sh.open_index_bin_levels(ix, positions="device")
        up.upload_index_bin(ix, positions=True)
        sets = _query_set(S, corpus, order, True)
        want = _answers(S, up, sets)
        _assert_same(_answers(S, sh, sets), want, "mode 3 against upload_index_bin")
        assert all(int(x[3].min()) > 0 for x in want[:3])           # every single term is found
        assert sum(int(x[3].sum()) for x in want[-3:]) > 0           # some phrase matches
        assert int(np.count_nonzero(want[-1][3][-6:])) > 0           # ... one naming an n-gram key among them

        def commit(level, lists, hi):
            o, d, t, np_, p = _csr(lists, level * LV, hi)
            sh.commit_level(level, corpus.doclen[level * LV:hi], o, d, t, nd if tiered else None, p, np_)

        def check(lists, n_docs, extra, what):
            fresh = _fresh(S, corpus, lists, nd if tiered else len(lists), n_docs, True)
            try:
                s = _query_set(S, corpus, lists, False, extra)
                _assert_same(_answers(S, sh, s), _answers(S, fresh, s), what)
            finally:
                fresh.close()

        commit(1, order, 2 * LV)  # the file's last level was incomplete: committed again, now full
        assert sh.incremental_info()[0] == 2
        check(order, 2 * LV, (), "after the re-commit of level 1")
        _assert_read(sh.read_level(1, 0, nd), _csr(order[:nd], LV, 2 * LV), "level 1 after its re-commit")
        _assert_read(sh.read_level(0, 0, nd), _csr(order[:nd], 0, LV), "level 0 after the re-commit of level 1")
        if tiered:  # what the open said the last level brought was exactly what the re-commit had to replace
            _assert_read(sh.read_sparse(0, len(order) - nd), _csr(order[nd:], 0, 2 * LV), "the tier after the re-commit")
        grown = order + ([] if tiered else [corpus.new_dense]) + corpus.new_rare
        commit(2, grown, N_FULL)
        assert sh.incremental_info()[0] == 3
        check(grown, N_FULL, tuple(range(len(order), len(grown))), "after the commit of level 2")
        if tiered:
            _assert_read(sh.read_sparse(0, len(grown) - nd), _csr(grown[nd:], 0, N_FULL), "the tier after the commit of level 2")
    finally:
        sh.close(); up.close(); ix.close()


def _replace_once(data, old, new):
    assert len(old) == len(new) and data.count(old) == 1, data.count(old)
    at = data.index(old)
    return data[:at] + new + data[at + len(old):]


def _record(positions):
    return RF.vint(len(positions)) + b"".join(RF.position_vint(x) for x in RF.delta_positions(positions))


def _defects(corpus):
    """{name: (file bytes, expected code)}: one defect each"""
    out = {}
    base = bytes(corpus.file)
    # the last stored gap of the posting that ends at exactly 65535, one larger: 65536 (the record stands in three blocks)
    rec = _record(_from_stored([60000, 5000, 533]))
    bad = rec[:-1] + bytes([rec[-1] + 1])
    assert base.count(rec) == 3
    at = base.index(rec)
    out["a position of 65536"] = (base[:at] + bad + base[at + len(rec):], -4)
    # a count VINT of 0 in front of 64 positions of one byte
    rec = _record(list(range(0, 192, 3)))
    assert base.count(rec) >= 1
    at = base.index(rec)
    out["record count 0"] = (base[:at] + bytes([0x80]) + base[at + 1:], -1)
    # a record alone in its segment whose count grows from 130 to 16383: its positions run over the quiet bytes behind it past byte_array_len
    rec = _record(corpus.tail_record)
    assert rec[:2] == RF.vint(130)
    out["positions past byte_array_len"] = (_replace_once(base, rec, RF.vint(16383) + rec[2:]), -1)
    # the first pointer of a block reaches back beyond the pointer range
    d = bytearray(base)
    _, body, cnt, pivot, ctp = _find_block(d, corpus.names["pcases0"].key, 0)
    rng_ = body + (ctp & 0x3FFFFFFF)
    assert pivot > 0 and not d[rng_ + 1] & 0x80 and (ctp & 0x3FFFFFFF) < 0x7FFF
    d[rng_:rng_ + 2] = bytes([0xFF, 0x7F])
    out["pointer beyond the pointer range"] = (bytes(d), -1)
    # twenty pointers of a block redirected to its 17000-position record: 21 * 17000 positions > byte_array_len + 4 * 65536
    d = bytearray(base)
    _, body, cnt, pivot, ctp = _find_block(d, corpus.names["big"].key, 0)
    rng_ = body + (ctp & 0x3FFFFFFF)
    assert pivot == 0 and cnt == 70 and not d[rng_ + 2] & 0x80
    for r in range(1, 21):
        d[rng_ + 3 * r:rng_ + 3 * r + 3] = d[rng_:rng_ + 3]
    out["twenty pointers to one long record"] = (bytes(d), -1)
    return out


def test_defective_files_are_refused_as_the_host_path_refuses_them(S, corpus):
    from seekstorm_amd import _native as N
    ix = _index_bin(S, corpus, True)
    order, nd = corpus.lists_of(ix, True)
    sh, other = S.Shard(0), S.Shard(0)
    try:
        sh.open_index_bin_levels(ix, positions="device")
        sets = _query_set(S, corpus, order, True)
        before, info, opened = _answers(S, sh, sets), sh.incremental_info()[:2], sh.open_info()
        for name, (data, code) in _defects(corpus).items():
            for tiered in (False, True):
                bad = _index_bin(S, corpus, tiered, data)
                with pytest.raises(N.SeekStormHipError) as host:
                    other.open_index_bin_levels(bad, positions="host")
                with pytest.raises(N.SeekStormHipError) as dev:
                    sh.open_index_bin_levels(bad, positions="device")
                bad.close()
                assert dev.value.code == code and host.value.code == code, (name, tiered, dev.value.code, host.value.code)
                assert sh.incremental_info()[:2] == info and sh.open_info() == opened, name
        _assert_same(_answers(S, sh, sets), before, "after the refusals")
        _assert_read(sh.read_level(1, 0, nd), _csr(order[:nd], LV, N_FILE), "level 1 after the refusals")
    finally:
        sh.close(); other.close(); ix.close()


def test_a_mode_outside_0_to_3_is_refused(S, corpus):
    from seekstorm_amd import _native as N
    ix = _index_bin(S, corpus, False)
    sh = S.Shard(0)
    try:
        with pytest.raises(N.SeekStormHipError) as e:
            sh.open_info()
        assert e.value.code == N.SS_ESTATE
        for mode in (4, -1, 7):
            with pytest.raises(N.SeekStormHipError) as e:
                sh.open_index_bin_levels(ix, positions=mode)
            assert e.value.code == N.SS_EINVAL and sh.incremental_info()[0] == 0
        sh.open_index_bin_levels(ix, positions=True)  # mode 1: the path the library prefers
        info, opened = sh.incremental_info()[:2], sh.open_info()
        assert opened[0] in (2, 3)
        with pytest.raises(N.SeekStormHipError) as e:
            sh.open_index_bin_levels(ix, positions=4)
        assert e.value.code == N.SS_EINVAL and sh.incremental_info()[:2] == info and sh.open_info() == opened
    finally:
        sh.close(); ix.close()
