"""Two small deterministic worlds for the phrase position check, and its definition (pure Python / numpy; no device, no oracle).

The check is written out in five kernels (bm25_phrase.hip, bm25_gallop.hip, bm25_sparse.hip, bm25_small.hip, bm25_phrase_bits.hip).
tests/test_gpu_phrase_positions.py drives all five over these worlds; tests/test_phrase_edge_world_cpu.py shows on the CPU that
the worlds are what they claim.

A world keeps   pos[term][doc] -> sorted positions   (several indexed fields: pos[term][(doc, field)]).  A doc matches the phrase
w_0 .. w_{n-1} when it holds every unique term and some p in pos[w_0][doc] has p + i in pos[w_i][doc] for every i -- on several
fields all of that inside ONE field, a listed one under a field filter.  NOT lists and tombstones are applied afterwards.  Expected
scores are those of the intersection of the unique terms by oracle/naive.py (bm25_exact / bm25f_exact: f32 factors, float64 sum).

Every FILL position is even, so fill never forms a phrase; everything that matches was planted.  Every named edge doc carries one
CASE (World.claims: case, doc, words, field filter, whether it matches).  Docs whose lists hold thousands of positions get the
longest length byte: their weights stay below those of the rich_miss docs (tf 40 in a doc of 8 words), which hold no phrase and
are the best-scoring docs of the intersection of A and B."""
import numpy as np

from oracle import naive

N_DOCS = 2 * 4096 + 77  # three sub-blocks, the last partial; no multiple of 64
SUB = 4096
LONG_LIST = 3000        # positions of the *_start cases (the binary search takes 12 steps)
T = ["T%d" % i for i in range(12)]
SIX = tuple(T[:6])
TWELVE = tuple(T)
LONG7 = tuple(T[:7] + T[:5])  # 12 words, 7 unique terms
GIANT, TINY = 255, 8          # length bytes: the longest; 8 words


class Phrase:
    def __init__(self, words, nots=(), filt=()):
        self.words, self.nots, self.filt = tuple(words), tuple(nots), tuple(filt)
        self.uniq = tuple(dict.fromkeys(self.words))

    @property
    def key(self):
        return (self.words, self.nots, self.filt)

    def __repr__(self):
        s = '"%s"' % " ".join(self.words)
        if self.nots:
            s += " -" + " -".join(self.nots)
        if self.filt:
            s += " fields %s" % (list(self.filt),)
        return s


class World:
    def __init__(self, name, n_fields):
        self.name, self.n_docs, self.n_fields = name, N_DOCS, n_fields
        self.pos = {}        # term -> doc (or (doc, field)) -> set of positions
        self.claims = []     # (case, doc, words, field filter, matches)
        self.slots = []      # (kind, term, doc): first_of_list / last_of_list / after_padding, in the untiered dense image
        self.label = {}      # doc -> case name, for failure messages
        self.reserved = set()  # docs that hold planted positions only: no fill
        self.table = []      # the phrases every route answers
        self.gone = []       # the tombstones of the "dead" runs
        self.dense, self.sparse = [], []  # the tiered form: its dense terms in order, then its sparse lists in order
        self.boost = None
        self.doclen = None
        self._cache = {}

    # ---- building
    def put(self, term, doc, positions, field=None):
        key = doc if self.n_fields == 1 else (doc, field)
        self.pos.setdefault(term, {}).setdefault(key, set()).update(int(p) for p in positions)
        self.reserved.add(doc)

    def case(self, name, doc, words, matches, filt=()):
        assert self.label.get(doc, "planted") in ("planted", name), ("a doc carries one case", doc, name, self.label[doc])
        self.label[doc] = name
        self.claims.append((name, doc, tuple(words), tuple(filt), bool(matches)))

    def plant(self, words, doc, start, field=None):
        for i, w in enumerate(words):
            self.put(w, doc, [start + i], field)
        self.label.setdefault(doc, "planted")

    # ---- reading
    @property
    def untiered(self):
        return self.dense + self.sparse

    def term_docs(self, term):
        if term not in self._cache:
            keys = self.pos[term]
            self._cache[term] = np.array(sorted(keys if self.n_fields == 1 else {d for d, _ in keys}), np.int64)
        return self._cache[term]

    def csr(self, terms):
        """the upload arrays of the terms in this order: offs, docs, [fields,] tfs, positions (u16, inside the field)"""
        offs, docs, fields, tfs, positions = [0], [], [], [], []
        for t in terms:
            for key in sorted(self.pos[t]):
                ps = sorted(self.pos[t][key])
                if self.n_fields == 1:
                    docs.append(key)
                else:
                    docs.append(key[0]); fields.append(key[1])
                tfs.append(len(ps)); positions += ps
            offs.append(len(docs))
        out = [np.asarray(offs, np.uint64), np.asarray(docs, np.uint32)]
        if self.n_fields > 1:
            out.append(np.asarray(fields, np.uint8))
        assert max(tfs) < 65536 and max(positions) < 65536
        return out + [np.asarray(tfs, np.uint16), np.asarray(positions, np.uint16)]

    def intersection(self, terms):
        out = None
        for t in dict.fromkeys(terms):
            out = self.term_docs(t) if out is None else np.intersect1d(out, self.term_docs(t))
        return out

    def doc_matches(self, doc, words, filt=()):
        """the definition, for one doc"""
        if self.n_fields == 1:
            lists = [self.pos[w].get(doc) for w in words]
            if any(l is None for l in lists):
                return False
            return any(all(p + i in lists[i] for i in range(1, len(words))) for p in lists[0])
        for f in range(self.n_fields):  # inside one field, a listed one
            if filt and f not in filt:
                continue
            lists = [self.pos[w].get((doc, f)) for w in words]
            if any(l is None for l in lists):
                continue
            if any(all(p + i in lists[i] for i in range(1, len(words))) for p in lists[0]):
                return True
        return False

    def matches(self, ph, dead=False):
        """the phrase's match set (doc ids ascending): the definition, then NOT lists, then tombstones"""
        key = ("m", ph.key, dead)
        if key not in self._cache:
            m = [int(d) for d in self.intersection(ph.uniq) if self.doc_matches(int(d), ph.words, ph.filt)]
            drop = set(self.gone) if dead else set()
            for t in ph.nots:
                drop |= set(self.term_docs(t).tolist())
            self._cache[key] = np.array([d for d in m if d not in drop], np.int64)
        return self._cache[key]

    def scores(self, uniq):
        """doc -> exact score of the intersection of the unique terms, in query order"""
        key = ("s", tuple(uniq))
        if key not in self._cache:
            if self.n_fields == 1:
                post = []
                for t in uniq:
                    d = self.term_docs(t)
                    post.append((d, np.array([len(self.pos[t][int(x)]) for x in d], np.uint16)))
                ids, sc = naive.bm25_exact(self.n_docs, self.doclen, post, True)
            else:
                ent = []
                for t in uniq:
                    keys = sorted(self.pos[t])
                    ent.append((np.array([k[0] for k in keys], np.int64), np.array([k[1] for k in keys], np.int64),
                                np.array([len(self.pos[t][k]) for k in keys], np.uint16)))
                ids, sc = naive.bm25f_exact(self.n_docs, self.doclen, self.boost, ent, True)
            self._cache[key] = dict(zip(ids.tolist(), sc.tolist()))
        return self._cache[key]

    def expected(self, ph, dead=False):
        """-> (docs, float64 scores) of every match, by (score descending, doc ascending)"""
        m = self.matches(ph, dead)
        sc = self.scores(ph.uniq)
        s = np.array([sc[int(d)] for d in m], np.float64)
        order = np.lexsort((m, -s))
        return m[order], s[order]

    def names(self, docs):
        return sorted("%s@%d" % (self.label.get(int(d), "fill"), int(d)) for d in docs)


# ------------------------------------------------------------------------------------------------ shared pieces
def _length_bytes(rng, n_docs):
    """ordinary docs: lengths between 2e4 and 4e6 words, around the average the giant docs leave behind"""
    ok = np.nonzero((naive.DLC >= 20_000) & (naive.DLC <= 4_000_000))[0]
    return rng.choice(ok, n_docs).astype(np.uint8)


def _pair_cases(W, x, y, at, field=None, long_list=LONG_LIST, tag=""):
    """the point cases of the two-word phrase "x y", one doc each; at: case -> doc.  -> the docs that hold a long list"""
    f = dict(field=field)
    giants = []
    for name, px, py, ok in (("zero", [0], [1], True), ("top", [65534], [65535], True), ("wrap", [65535], [0], False),
                             ("sign", [32767], [32768], True), ("same", [10], [10], False), ("rev", [11], [10], False),
                             ("gap", [10], [12], False), ("gap_back", [10], [9], False),
                             # the same edges inside lists that span the sign bit: a one-element list is found by any compare, signed or not
                             ("sign_span", [6, 32767], [2, 20000, 32768, 50000], True), ("top_span", [8, 65534], [4, 30000, 65535], True)):
        if name in at:
            W.put(x, at[name], px, **f); W.put(y, at[name], py, **f)
            W.case(tag + name, at[name], (x, y), ok)
            if name == "rev" and not tag:  # ("B A" is in the table; the other pairs' reversals are not)
                W.claims.append((tag + name, at[name], (y, x), (), True))
    n = long_list
    for name, hit in (("last_start", n - 1), ("first_start", 0), ("mid_start", n // 2)):
        if name in at:
            # x = {3 i}, y = {3 i + 2}: no start finds its successor -- but for start 3 hit, where y holds 3 hit + 1 instead
            W.put(x, at[name], [3 * i for i in range(n)], **f)
            W.put(y, at[name], [3 * i + (1 if i == hit else 2) for i in range(n)], **f)
            W.case(tag + name, at[name], (x, y), True)
            giants.append(at[name])
    return giants


def _fill(W, rng, term, n, field_of=None):
    """n docs outside the reserved ones, tf 1 .. 3, EVEN positions below 2000"""
    free = np.array(sorted(set(range(W.n_docs)) - W.reserved), np.int64)
    for d in rng.choice(free, n, replace=False):
        tf = int(rng.integers(1, 4))
        ps = (2 * rng.choice(1000, tf, replace=False)).tolist()
        key = int(d) if W.n_fields == 1 else (int(d), int(field_of(rng)))
        W.pos.setdefault(term, {}).setdefault(key, set()).update(ps)


def _segment(W, term, sub):
    return [d for d in W.term_docs(term).tolist() if d // SUB == sub]


def _pad_segments(W, term, subs):
    """drop fill postings until the term's segments of these sub-blocks are no multiple of 4 postings: each ends in NULL padding"""
    for sub in subs:
        while len(_segment(W, term, sub)) % 4 == 0:
            victim = max(d for d in _segment(W, term, sub) if d not in W.reserved)
            for key in [k for k in W.pos[term] if (k if W.n_fields == 1 else k[0]) == victim]:
                del W.pos[term][key]
            W._cache.pop(term, None)


# ------------------------------------------------------------------------------------------------ World 1
def build_world1():
    """one indexed field, u16 positions.  |D| < |E| < |A| < |B| < |C| < |F|; T0 .. T11 serve the long phrases; F is the NOT list"""
    W = World("one field", 1)
    rng = np.random.default_rng(20_260_001)
    n = N_DOCS
    giants = []
    # ---- "A B" at the doc-id edges: 0, 63, 64, 65, 4095, 4096, 8191, 8192, n - 1
    giants += _pair_cases(W, "A", "B", {"zero": 0, "top": 63, "wrap": 64, "sign": 65, "same": 4095, "last_start": 4096, "gap": 8191,
                                        "first_start": 8192, "mid_start": n - 1, "rev": 100, "gap_back": 101, "sign_span": 66, "top_span": 62})
    for t in ("A", "B"):
        W.slots += [("first_of_list", t, 0), ("last_of_list", t, n - 1), ("after_padding", t, 4096), ("after_padding", t, 8192)]
    # ---- "B C" and "C A": the other word orders of the tiers (sparse-dense, dense-sparse), and C as a driven / driving dense list
    giants += _pair_cases(W, "B", "C", {"zero": 1, "sign": 4097, "top": n - 2, "wrap": 2050, "same": 2051, "gap": 2052, "last_start": 2053,
                                        "rev": 2054, "sign_span": 2055, "top_span": 2056}, tag="bc_")
    W.slots += [("first_of_list", "C", 1), ("after_padding", "C", 4097), ("last_of_list", "C", n - 2)]
    giants += _pair_cases(W, "C", "A", {"zero": 6000, "top": 6001, "sign": 6002, "wrap": 6003, "same": 6004, "gap": 6005, "last_start": 6006,
                                        "rev": 6007, "sign_span": 6008, "top_span": 6009}, tag="ca_")
    # ---- second_try: the first start passes B and fails C by one, a later start passes both
    W.put("A", 200, [20, 40]); W.put("B", 200, [21, 41]); W.put("C", 200, [23, 42])
    W.case("second_try", 200, ("A", "B", "C"), True)
    W.put("A", 201, [20, 40]); W.put("B", 201, [21, 41]); W.put("C", 201, [23, 43])  # ... and its sibling where no start does
    W.case("second_try_miss", 201, ("A", "B", "C"), False)
    # ---- repeated words
    W.put("A", 300, [50, 51]); W.case("aa", 300, ("A", "A"), True); W.claims.append(("aa", 300, ("A", "A", "A"), (), False))
    W.put("A", 301, [50, 52]); W.case("aa_gap", 301, ("A", "A"), False)
    W.put("A", 302, [50, 51, 52]); W.case("aaa", 302, ("A", "A", "A"), True)
    W.put("A", 303, [60, 62]); W.put("B", 303, [61]); W.case("aba", 303, ("A", "B", "A"), True)
    W.put("A", 304, [60]); W.put("B", 304, [61]); W.case("aba_short", 304, ("A", "B", "A"), False)
    # ---- last_word_off: every word in place but the last, which is one too far; a sibling doc is correct
    for words, bad, good in ((SIX, 400, 401), (TWELVE, 402, 403), (LONG7, 404, 405)):
        W.plant(words, good, 100)
        W.plant(words[:-1], bad, 100)
        W.put(words[-1], bad, [100 + len(words)])
        W.case("last_word_off", bad, words, False)
        W.case("last_word_ok", good, words, True)
    # ---- rich_miss: tf 40 of A and of B in docs of 8 words, no phrase: the best-scoring docs of the intersection
    W.rich = [500 + 251 * i for i in range(30)]
    assert not set(W.rich) & W.reserved
    for d in W.rich:
        W.put("A", d, [4 * i for i in range(40)]); W.put("B", d, [4 * i + 2 for i in range(40)])
        W.case("rich_miss", d, ("A", "B"), False)
    # ---- planted matches in docs of their own (starts odd and even)
    free = [int(d) for d in rng.permutation(n) if int(d) not in W.reserved and 70 < int(d) < n - 70]
    take = iter(free)
    W.not_f, W.not_d = [65], []
    for words, cnt in ((("A", "B"), 25), (("B", "A"), 15), (("A", "B", "C"), 10), (("B", "C"), 20), (("C", "A"), 15), (("C", "F"), 15),
                       (("A", "D"), 10), (("D", "A", "B"), 8), (("A", "B", "E"), 8), (("D", "A", "B", "E"), 6), (("A", "A"), 6),
                       (("A", "B", "A"), 6), (SIX, 10), (TWELVE, 6), (LONG7, 6)):
        for j in range(cnt):
            d = next(take)
            W.plant(words, d, int(rng.integers(0, 1500)))
            if words in (("A", "B"), ("B", "C")) and j < 5:
                W.not_f.append(d)
            if words == ("D", "A", "B"):
                W.not_d.append(d)
    for d in W.not_f:  # matches of "A B" that the NOT list F removes (an even position, like all fill)
        W.put("F", d, [1998])
    # ---- fill: random docs outside the reserved ones, even positions
    for t, cnt in (("D", 100), ("E", 130), ("A", 300), ("B", 500), ("C", 2000), ("F", 2600)):
        _fill(W, rng, t, cnt)
    for i, t in enumerate(T):
        _fill(W, rng, t, 250 + 15 * i)
    for t in ("A", "B", "C"):
        _pad_segments(W, t, (0, 1))
    # ---- lengths
    W.doclen = _length_bytes(rng, n)
    W.doclen[giants] = GIANT
    W.doclen[W.rich] = TINY
    W.giants = giants
    W.dense, W.sparse = ["C"] + T + ["F"], ["A", "B", "D", "E"]  # (A first: its doc 0 is the sparse tier's very first posting)
    W.sparse_terms = set(W.sparse)
    W.table = [Phrase(w) for w in (("A", "B"), ("B", "A"), ("A", "A"), ("A", "A", "A"), ("A", "B", "A"), ("A", "B", "C"), ("B", "C"), ("C", "A"),
                                   ("C", "F"), ("A", "D"), ("D", "A", "B"), ("A", "B", "E"), ("D", "A", "B", "E"), SIX, TWELVE, LONG7)]
    W.table += [Phrase(("A", "B"), ("F",)), Phrase(("A", "B"), ("D",)), Phrase(("B", "C"), ("F", "D"))]
    W.gone = sorted({63, 8192, W.rich[3], W.not_d[0], 403, 2053} | set(range(7, n, 97)))
    W.gone_edges = [63, 8192]  # two matching edge docs of "A B"
    W.drivers = {"A": ("A", "B"), "B": ("B", "C"), "C": ("C", "F"), "D": ("A", "D"), "E": ("A", "B", "E")}  # shortest list -> a phrase it drives
    return W


# ------------------------------------------------------------------------------------------------ World 2
BOOST = np.array([2.0, 1.0, 0.5], np.float32)
T7 = tuple(T[:7])


def build_world2():
    """three indexed fields, field-tagged u32 positions on the device (merged lists); G is the NOT list"""
    W = World("three fields", 3)
    rng = np.random.default_rng(20_260_002)
    n = N_DOCS
    W.boost = BOOST
    for x, y, base, tag in (("A", "B", 0, ""), ("B", "C", 2000, "bc_"), ("C", "A", 6000, "ca_")):
        # "A B" at the doc-id edges, the other two pairs in docs base .. base + 7
        at = [0, 63, 65, 4096, 64, 4095, 8192, n - 1, 66, 62] if base == 0 else [base + i for i in range(10)]
        _pair_cases(W, x, y, {"sign_span": at[8]}, field=1, tag=tag)
        _pair_cases(W, x, y, {"top_span": at[9]}, field=2, tag=tag)
        _pair_cases(W, x, y, {"zero": at[0]}, field=0, tag=tag)
        _pair_cases(W, x, y, {"top": at[1]}, field=2, tag=tag)
        _pair_cases(W, x, y, {"sign": at[2]}, field=1, tag=tag)
        _pair_cases(W, x, y, {"last_start": at[3]}, field=1, long_list=1000, tag=tag)
        d = at[4]  # the seam: the last position of field 0, then position 0 of field 1
        W.put(x, d, [65535], 0); W.put(y, d, [0], 1); W.case(tag + "wrap", d, (x, y), False)
        d = at[5]  # consecutive numbers in different fields
        W.put(x, d, [200], 0); W.put(y, d, [201], 2); W.case(tag + "cross", d, (x, y), False)
        d = at[6]  # in fields 0 and 2: not under a filter that lists field 1 only
        W.put(x, d, [30], 0); W.put(y, d, [31], 0); W.put(x, d, [40], 2); W.put(y, d, [41], 2)
        W.case(tag + "in_0_and_2", d, (x, y), True)
        W.claims += [(tag + "in_0_and_2", d, (x, y), (1,), False), (tag + "in_0_and_2", d, (x, y), (2,), True), (tag + "in_0_and_2", d, (x, y), (0, 2), True)]
        d = at[7]  # in field 1 only
        W.put(x, d, [5], 1); W.put(y, d, [6], 1)
        W.case(tag + "in_1", d, (x, y), True)
        W.claims += [(tag + "in_1", d, (x, y), (1,), True), (tag + "in_1", d, (x, y), (2,), False), (tag + "in_1", d, (x, y), (0, 2), False)]
    for t in ("A", "B"):
        W.slots += [("first_of_list", t, 0), ("last_of_list", t, n - 1), ("after_padding", t, 4096), ("after_padding", t, 8192)]
    # a seven-term phrase in field 1, its last word one too far in a sibling; a word of the phrase in ANOTHER field does not help
    W.plant(T7, 401, 100, 1); W.case("last_word_ok", 401, T7, True)
    W.plant(T7[:-1], 400, 100, 1); W.put(T7[-1], 400, [107], 1); W.put(T7[-1], 400, [106], 2); W.case("last_word_off", 400, T7, False)
    free = [int(d) for d in rng.permutation(n) if int(d) not in W.reserved and 70 < int(d) < n - 70]
    take = iter(free)
    W.not_g = [65]
    for words, cnt in ((("A", "B"), 24), (("B", "A"), 12), (("B", "C"), 18), (("C", "A"), 12), (("A", "B", "C"), 9), (("C", "G"), 12), (T7, 9)):
        for j in range(cnt):
            d = next(take)
            W.plant(words, d, int(rng.integers(0, 1500)), j % 3)
            if words == ("A", "B") and j < 5:
                W.not_g.append(d)
    for d in W.not_g:
        W.put("G", d, [1998], 0)
    field_of = lambda r: r.integers(0, 3)
    for t, cnt in (("A", 300), ("B", 500), ("C", 2000), ("G", 2600)):
        _fill(W, rng, t, cnt, field_of)
        _fill(W, rng, t, cnt // 4, field_of)  # (some docs hold the term in two fields)
    for i, t in enumerate(T7):
        _fill(W, rng, t, 250 + 15 * i, field_of)
    for t in ("A", "B"):
        _pad_segments(W, t, (0, 1))
    ok = np.nonzero((naive.DLC >= 20) & (naive.DLC <= 70_000))[0]
    W.doclen = rng.choice(ok, (3, n)).astype(np.uint8)
    W.dense, W.sparse = ["C"] + list(T7) + ["G"], ["A", "B"]
    W.sparse_terms = set(W.sparse)
    W.table = [Phrase(("A", "B")), Phrase(("A", "B"), filt=(1,)), Phrase(("A", "B"), filt=(2,)), Phrase(("A", "B"), filt=(0, 2)), Phrase(("B", "A")),
               Phrase(("B", "C")), Phrase(("B", "C"), filt=(1,)), Phrase(("C", "A")), Phrase(("C", "A"), filt=(0, 2)), Phrase(("A", "B", "C")),
               Phrase(("C", "G")), Phrase(("C", "G"), filt=(1,)), Phrase(T7), Phrase(T7, filt=(1,)), Phrase(T7, filt=(0, 2)),
               Phrase(("A", "B"), ("G",)), Phrase(("A", "B"), ("G",), (1, 2))]
    W.gone = sorted({63, 8192, 401, 2003} | set(range(7, n, 97)))
    W.gone_edges = [63, 8192]
    W.drivers = {"A": ("A", "B"), "B": ("B", "C"), "C": ("C", "G")}
    return W


_WORLDS = {}


def world(which):
    """the worlds are built once per process and never changed"""
    if which not in _WORLDS:
        _WORLDS[which] = build_world1() if which == 1 else build_world2()
    return _WORLDS[which]
