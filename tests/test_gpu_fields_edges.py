"""Images with several indexed fields (BM25F) and the generic galloping kernel (bm25_gallop.hip), doc for doc against
naive.bm25f_exact -- the crate's f32 factors, products and sums in float64 -- with the checks of test_gpu_score_edges (_check: no doc twice,
every doc a match, every score within REL = 1e-4 of ITS exact score, the docs above the k-th score's tie band the reference's, bit-equal
groups in doc-id order; exact_ties: the very list of the reference), and exact totals for TopkCount and Count.

Small BUILT worlds (n_docs = 3 * 4096 + 37: three full sub-blocks and a partial one), 3 indexed fields.  A doc has one of six weight
classes (two length bytes per field x tf 1 / 2 / 3, the same in every field and list) and one of four field patterns by doc % 4 (all
three fields / the last only / the first only / fields 1 and 2): few distinct scores, many exact ties.  exact_ties is asked of a query
only where the CPU proves (FWorld.exact) that its distinct reference scores lie more than twice the tie band apart AND that equal
reference scores belong to docs with the same per-(term, field) (tf, length byte) signature -- such docs read the same codes in the same
order in every kernel.
  M   boosts [2, 1, 0.5]: merged lists are built.  The first `nd` terms are the dense image, S1 .. S3 go in through append_sparse_fields.
  P   the same postings (dense ones) under boosts [4096, 1, 1 / 4096]: no merged lists, every query reads (term, field) lists.
  P64 6 sub-blocks, ten terms in all three fields of nearly every doc: the shortest term's field lists sum to > 65 536 postings (64 shares).
Lists (ids in this order): E0 / E1 / E2 whose (term, field) segments per sub-block hold 0, 4 (one full 16-byte unit) and 5 (a unit, a
posting, padding) postings -- E0 short (it DRIVES: NULL padding and empty directory segments inside a driver's image), E1 / E2 with a bulk
list in field 2 (they are PROBED: under a filter on M and always on P dense_find walks the small segments), E1 without any posting in
field 1; W, the probe list: every sub-block's local docs 0 and 4095, every small segment's first and last posting and the doc behind the
last; X0 .. X9 small NOT lists; G0 .. G23 wide lists (G0 .. G12: 25 - 50 % of the docs) over a shared core, G0 strictly the shortest
(a query names it first and last); F0 .. F7 in more than half of the docs with tf 9 | 10 in the doc's lowest field and >= 10 elsewhere,
and the reverse (all_terms_frequent); H1 / H2 drivers of some 1 400 / 2 200 docs; Z1 never in field 1 (it passes the filter (1, 2) through
field 2 only); Z0 without a posting; sparse S1, S2 (never in field 1), S3.  Postings stand on docs 0, 63, 64, 4095, 4096, 8191, 8192
and n_docs - 1 (the core holds them).

Shares: P = min(64, max(1, longest_driver / 1024), 8192 / nq) waves per query, wave `part` of a driver list of `chunks` 64-posting steps
walks [((chunks * part) / P) << 6, ((chunks * (part + 1)) / P) << 6).  _share_docs computes from the padded image layout (segments per
4096 docs, padded to 4 postings) the docs in the first and last slot of every share and next to NULL padding; with a few docs the driver
holds in two field lists they get the top weight class, the core holds them, and a CPU test shows they rank.

Routing (bm25_shape_of), asserted with generic_batches() query by query on both sides of every seam: filtered (M) or any (P)
intersections of 8 | 9 terms, 8 terms with 2 | 3 NOT terms (30 | 33 (term, field) lists around BM_MAX_VTERMS = 32), one term with 9 | 10
NOT terms, all_terms_frequent with 7 | 8 terms on M; a query naming a sparse term runs bm25_sparse.hip's gate, never gallop.

The claim of bm25_gallop.hip's header -- bit-identical to the specialised kernels where both can answer -- is pinned at the end: phrases
at k = 128 (native) | 129 (gallop), a phrase on a shard whose rationed probe rows leave its lists row-less against the full shard, and
all_terms_frequent intersections of 7 (native) | 8 (gallop) terms whose eighth list holds every doc with an idf of 1e-30: fmaf(1e-30, w,
s) == s for every score s of the 7-term chain, so the two answers must be equal bit for bit -- that comparison is exact on the CPU side.
Phrase match sets are also checked against a brute-force numpy match over the texts.

The tests not marked gpu prove on the CPU (naive only) that the worlds hold what they are built for and that _check rejects a duplicated
doc, a doc answered under a one-field score and a tie broken the wrong way."""
import collections
import types

import numpy as np
import pytest

from oracle import naive
from test_gpu_score_edges import REL, _check

N_DOCS = 3 * 4096 + 37
NF = 3
BOOST_M = (2.0, 1.0, 0.5)
BOOST_P = (4096.0, 1.0, 1.0 / 4096.0)
# every KPL instance of the galloping kernel on both sides of its seam (64 | 65: KPL 1 | 2, 128 | 129: 2 | 4, 256 | 257: 4 | 16) and its largest k
KS = (1, 10, 64, 65, 128, 129, 256, 257, 1024)
K_DEEP = 1500   # beyond SS_MAX_K: the deep-page pass, run once per world
SEAM = [0, 63, 64, 4095, 4096, 8191, 8192, N_DOCS - 1]
TOMB = [0, 63, 64, 4095, 4096, N_DOCS - 1]
FILTERS = ((), (0,), (1, 2))
PAT = np.array([[1, 1, 1], [0, 0, 1], [1, 0, 0], [0, 1, 1]], bool)     # fields of a doc, by doc % 4
PAT_Z = np.array([[1, 0, 1], [0, 0, 1], [1, 0, 1], [1, 0, 0]], bool)   # ... of Z1 and S2: never field 1
LENS = ((10, 300), (6, 200), (8, 120))   # the two lengths of every field (field 1 the shorter: w1 > w0 in every class)
TOP = 2   # the weight class of the short length and tf 3: the highest weight in every field
BM_MAX_VTERMS = 32

Q = collections.namedtuple("Q", "terms op_and nots filt freq")


def _b4(x):
    return naive.int_to_byte4(int(x))


class FCorpus:
    """Corpus of test_gpu_score_edges over several indexed fields: entries (docs, fields, tfs) per term, sorted by (doc, field)"""
    def __init__(self, n_docs, doclen_fields, boost, entries):
        self.n_docs, self.doclen, self.boost = n_docs, np.asarray(doclen_fields, np.uint8), np.asarray(boost, np.float32)
        self.entries = [(np.asarray(d, np.uint32), np.asarray(f, np.uint8), np.asarray(t, np.uint16)) for d, f, t in entries]
        self.offs = np.zeros(len(entries) + 1, np.uint64)
        self.offs[1:] = np.cumsum([len(e[0]) for e in self.entries])
        self.docs = np.concatenate([e[0] for e in self.entries])
        self.fields = np.concatenate([e[1] for e in self.entries])
        self.tfs = np.concatenate([e[2] for e in self.entries])
        self._ref = {}

    def ref(self, terms, op_and, nots=(), deleted=(), field_filter=(), frequent=False):
        """-> (ids ascending, their exact scores, ids by (score desc, id asc), the scores in that order); frequent: the RANKED docs"""
        deleted = np.asarray(deleted, np.int64)
        key = (tuple(terms), op_and, tuple(nots), deleted.tobytes(), tuple(field_filter), frequent)
        if key not in self._ref:
            ent = [self.entries[t] for t in terms]
            if frequent:
                assert op_and and not nots and not field_filter
                ids, sc, _ = naive.bm25f_shortcut_exact(self.n_docs, self.doclen, self.boost, ent, deleted=deleted)
            else:
                ids, sc = naive.bm25f_exact(self.n_docs, self.doclen, self.boost, ent, op_and, not_docs=[self.entries[t][0] for t in nots],
                                            deleted=deleted, field_filter=field_filter)
            order = np.lexsort((ids, -sc))
            self._ref[key] = (ids, sc, ids[order].astype(np.int64), sc[order])
        return self._ref[key]

    def view(self, field_filter=(), frequent=False):
        """what _check reads: ref(terms, op_and, nots, deleted) under this filter / rule"""
        return types.SimpleNamespace(ref=lambda terms, op_and, nots=(), deleted=(): self.ref(terms, op_and, nots, deleted, field_filter, frequent))


def _entries(per_field, tf):
    """per_field: the docs of every field list; tf: per-doc array, or f(docs, fields, first entry of its doc) -> tfs"""
    dd = np.concatenate([np.asarray(d, np.int64) for d in per_field])
    ff = np.concatenate([np.full(len(d), f, np.int64) for f, d in enumerate(per_field)])
    o = np.lexsort((ff, dd))
    dd, ff = dd[o], ff[o]
    first = np.ones(len(dd), bool)
    first[1:] = dd[1:] != dd[:-1]
    return dd, ff, (tf(dd, ff, first) if callable(tf) else tf[dd])


def _by_pattern(docs, table=PAT):
    docs = np.unique(np.asarray(docs, np.int64))
    return [docs[table[docs % 4, f]] for f in range(NF)]


def _padded(docs, n_docs):
    """the image of one list: its segments per 4096 docs, each padded with NULL (-1) to a multiple of 4 postings"""
    docs = np.asarray(docs, np.int64)
    out = [np.zeros(0, np.int64)]
    for sb in range((n_docs + 4095) // 4096):
        seg = docs[(docs >> 12) == sb]
        out += [seg, np.full((-len(seg)) % 4, -1, np.int64)]
    return np.concatenate(out)


def _shares(longest_driver, nq):
    return max(1, min(min(64, max(1, longest_driver // 1024)), max(1, 8192 // nq)))


def _share_docs(image, P):
    """the docs in the first and last slot of every share of a driver's image, and those next to NULL padding"""
    chunks = (len(image) + 63) >> 6
    pick = set()
    for part in range(P):
        b, e = ((chunks * part) // P) << 6, min(((chunks * (part + 1)) // P) << 6, len(image))
        live = np.nonzero(image[b:e] >= 0)[0]
        if len(live):
            pick |= {int(image[b + live[0]]), int(image[b + live[-1]])}
    for i in np.nonzero(image < 0)[0]:
        for j in (i - 1, i + 1):
            if 0 <= j < len(image) and image[j] >= 0:
                pick.add(int(image[j]))
    return pick


def _driver_images(per_field, merged, n_docs):
    """the lists a dense driver is walked by: its merged list, or its field lists one after the other"""
    if merged:
        return [_padded(np.unique(np.concatenate(per_field)), n_docs)]
    return [_padded(d, n_docs) for d in per_field]


def _driver_postings(per_field, merged):
    return len(np.unique(np.concatenate(per_field))) if merged else sum(len(d) for d in per_field)


E_SEGS = {  # (term, field) lists by sub-block: local docs -- segments of 0, 4, 5 (and 1, 2) postings; "bulk": 300 random docs and BULK_W
    "E0": [{0: [0, 9, 10, 11, 4095], 2: [1, 2, 3, 4094]}, {}, {1: [0, 1, 2, 4095], 3: [0, 1, 2, 3, 36]}],
    "E1": [{0: [0, 17, 100, 4095], 1: [4, 6, 7, 8, 10], 3: [36]}, {}, "bulk"],
    "E2": [{0: [0, 1000, 4095]}, {1: [0, 1, 2, 4095], 2: [0, 2000, 3000, 4000, 4095], 3: [0, 1, 2, 3]}, "bulk"],
}
BULK_W = [1000, 5000, 9000]   # docs of W in the bulk lists (all three fields hold them, no tombstone: [W, E1 ..] matches under every filter)
SHARE_DRIVERS = ("G0", "H1", "H2")


def _seg_docs(segs):
    return np.array(sorted(sb * 4096 + x for sb, loc in segs.items() for x in loc), np.int64)


def _f_tf(index):
    """tf of the frequent lists: by (doc / 4) % 4 -- 9 in the doc's lowest field and 60 elsewhere (the best docs, were they ranked) | 10 and 9 | 10 and 10 | 12 and 11; F3
    alone has 9 in the lowest field of the docs with doc % 64 == 7"""
    def tf(dd, ff, first):
        mode = (dd // 4) % 4
        t = np.where(first, np.array([9, 10, 10, 12])[mode], np.array([60, 9, 10, 11])[mode])
        if index == 3:
            t = np.where(first & (dd % 64 == 7), 9, t)
        return t
    return tf


def _blueprint():
    """the postings of M and P: {name: (docs per field, tf rule)} in term-id order, the doc classes, the share-seam docs"""
    rng = np.random.default_rng(303)
    n = N_DOCS
    pick = lambda m: rng.choice(n, int(m), replace=False)
    lists = {}
    small = set()
    for name, fl in E_SEGS.items():
        per = []
        for segs in fl:
            if segs == "bulk":
                per.append(np.union1d(pick(300), BULK_W).astype(np.int64))
            else:
                per.append(_seg_docs(segs))
                small |= set(per[-1].tolist())
        lists[name] = (per, None)
    probe = {63, 64, 1000, 5000, 9000, 12300}   # (the last four: in no small segment, so that W without E0 / E1 / E2 keeps docs)
    for sb in range(4):
        probe |= {sb * 4096, min(sb * 4096 + 4095, n - 1)}
    for fl in E_SEGS.values():
        for segs in fl:
            if segs == "bulk":
                continue
            for sb, loc in segs.items():
                probe |= {sb * 4096 + loc[0], sb * 4096 + loc[-1]}
                if loc[-1] + 1 < 4096 and sb * 4096 + loc[-1] + 1 < n:
                    probe.add(sb * 4096 + loc[-1] + 1)
    w_docs = np.array(sorted(probe), np.int64)
    lists["W"] = ([w_docs] * NF, None)   # (in every field: it passes every filter)
    for i in range(10):
        lists[f"X{i}"] = (_by_pattern(np.union1d(pick(60), w_docs[i::10][:1])), None)
    big = pick(1500)   # the shared core: every wide list holds it, the drivers H1 / H2 most of it -- intersections keep > 257 docs under every filter
    edge = np.unique(np.concatenate([SEAM, w_docs, sorted(small)])).astype(np.int64)
    base = np.union1d(edge, big)
    drivers = {"G0": np.union1d(base, pick(0.16 * n)), "H1": np.unique(np.concatenate([edge, big[:1000], pick(300)])),
               "H2": np.unique(np.concatenate([edge, big[:1400], pick(800)]))}
    special = set()
    for name in SHARE_DRIVERS:
        per = _by_pattern(drivers[name])
        for merged in (True, False):
            for image in _driver_images(per, merged, n):
                special |= _share_docs(image, _shares(_driver_postings(per, merged), 1))
        for r in (0, 3):   # docs the driver holds in several field lists
            special |= set(int(x) for x in drivers[name][drivers[name] % 4 == r][5:8])
    special = np.array(sorted(special), np.int64)
    core = np.union1d(base, special)
    lists["G0"] = (_by_pattern(drivers["G0"]), None)
    for i in range(1, 24):
        lists[f"G{i}"] = (_by_pattern(np.union1d(core, pick((0.17 + 0.01 * i) * n))), None)
    for i in range(8):
        lists[f"F{i}"] = (_by_pattern(np.union1d(core, pick((0.45 + 0.02 * i) * n))), _f_tf(i))
    lists["H1"] = (_by_pattern(drivers["H1"]), None)
    lists["H2"] = (_by_pattern(drivers["H2"]), None)
    lists["Z1"] = (_by_pattern(np.union1d(core, pick(0.1 * n)), PAT_Z), None)
    lists["Z0"] = ([np.zeros(0, np.int64)] * NF, None)
    nd = len(lists)
    s1 = np.union1d(core[::7], pick(300))
    lists["S1"] = (_by_pattern(s1), None)
    lists["S2"] = (_by_pattern(np.union1d(core[::5], pick(250)), PAT_Z), None)
    lists["S3"] = (_by_pattern(np.union1d(s1[::6], pick(200))), None)
    cls = rng.choice([0, 1, 3, 4, 5], n)
    cls[special] = TOP
    return lists, nd, cls, special


class FWorld:
    def __init__(self, kind, n_docs, boost, lists, nd, cls, special):
        self.kind, self.merged = kind, kind == "M"
        self.names = list(lists)[:len(lists) if self.merged else nd]   # (P: the dense tier only)
        self.nd = nd
        self.id = {name: i for i, name in enumerate(self.names)}
        self.per_field = {name: lists[name][0] for name in self.names}
        self.cls, self.special = cls, special
        dl = np.stack([np.array([_b4(x) for x in LENS[f]], np.uint8)[cls // 3] for f in range(NF)])
        tf_of = (1 + cls % 3).astype(np.int64)
        self.c = FCorpus(n_docs, dl, boost, [_entries(lists[name][0], lists[name][1] or tf_of) for name in self.names])
        self.deleted = ()
        self._sig, self._exact = {}, {}

    def docs(self, name):
        return np.unique(np.concatenate(self.per_field[name]))

    def q(self, terms, nots=(), filt=(), op_and=True, freq=False):
        return Q(tuple(self.id[t] for t in terms), op_and, tuple(self.id[t] for t in nots), tuple(filt), freq)

    def label(self, x):
        return f"{self.kind} {'AND' if x.op_and else 'OR'} {[self.names[t] for t in x.terms]} NOT {[self.names[t] for t in x.nots]} filter {x.filt}" \
               f"{' all_terms_frequent' if x.freq else ''}"

    def driver_postings(self, x):
        """bm25_shape_of's driver_len: the fewest postings of a scored term (its merged list, or its field lists together)"""
        return min(_driver_postings(self.per_field[self.names[t]], self.merged) for t in x.terms)

    def gallop(self, x, k=10):
        """bm25_shape_of restated: does the query go to the generic galloping kernel?"""
        n_terms, n_all = len(x.terms), len(x.terms) + len(x.nots)
        is_and = x.op_and and n_terms > 1
        if x.freq and k == 10 and is_and and not x.filt and n_terms > 7:
            return True
        any_sparse = any(t >= self.nd for t in x.terms + x.nots)
        return bool((x.filt or not self.merged) and not any_sparse and (n_all * NF > BM_MAX_VTERMS or (is_and and n_terms > 8)))

    def ref(self, x, deleted=(), frequent=False):
        return self.c.ref(x.terms, x.op_and, x.nots, deleted, x.filt, frequent)

    def signature(self, t):
        """(tf << 8 | length byte) + 1 of every doc in every field list of term t, 0 where the list does not hold the doc"""
        if t not in self._sig:
            d, f, tf = self.c.entries[t]
            s = np.zeros((NF, self.c.n_docs), np.int64)
            s[f, d] = ((tf.astype(np.int64) << 8) | self.c.doclen[f, d]) + 1
            self._sig[t] = s
        return self._sig[t]

    def exact(self, x, deleted=(), frequent=False):
        """the CPU's proof for exact_ties: distinct reference scores more than twice the tie band apart, equal ones only between docs of one
        per-(term, field) (tf, length byte) signature"""
        key = (x, np.asarray(deleted, np.int64).tobytes(), frequent)
        if key not in self._exact:
            ids, sc, rd, rs = self.ref(x, deleted, frequent)
            u = np.unique(rs)
            ok = len(u) < 2 or float((np.diff(u) / u[1:]).min()) > 2 * REL
            if ok and len(rd) > 1:
                sig = np.concatenate([self.signature(t)[:, rd] for t in x.terms]).T
                ok = bool(np.all((sig[1:] == sig[:-1]).all(axis=1)[rs[1:] == rs[:-1]]))
            self._exact[key] = ok
        return self._exact[key]


_WORLDS = {}


def _world(kind):
    if kind not in _WORLDS:
        if kind == "P64":
            _WORLDS[kind] = _build_p64()
        else:
            if "blueprint" not in _WORLDS:
                _WORLDS["blueprint"] = _blueprint()
            lists, nd, cls, special = _WORLDS["blueprint"]
            w = FWorld(kind, N_DOCS, BOOST_M if kind == "M" else BOOST_P, lists, nd, cls, special)
            w.deleted = np.unique(np.concatenate([TOMB, w.docs("G0")[::3], w.docs("E0")[2::3]]))   # seams, every third doc of a driver
            _WORLDS[kind] = w
    return _WORLDS[kind]


G = lambda a, b: [f"G{i}" for i in range(a, b)]
A8 = G(1, 9)
NOT10 = ["E1", "E2", "E0"] + [f"X{i}" for i in range(7)]


def _seam_cases():
    """(terms, NOT terms, beyond the seam?): each pair stands on both sides of a seam of bm25_shape_of -- beyond it a query over per-field
    lists (any query of P, a filtered one of M) is the galloping kernel's"""
    return [
        (A8, [], False), (A8 + ["G9"], [], True),                                   # 8 | 9 scored terms
        (A8, ["X0", "X1"], False), (A8, ["X0", "X1", "X2"], True),                  # 30 | 33 (term, field) lists
        (["W"], NOT10[:9], False), (["W"], NOT10, True),                            # one term, 9 | 10 NOT terms (NOT lists with small segments)
        (["Z1"], [f"X{i}" for i in range(9)], False), (["Z1"], [f"X{i}" for i in range(10)], True),
        (["G0"] + A8, [], True), (A8 + ["G0"], [], True),                           # the driver first and last
        (["W", "E1"] + G(1, 8), [], True), (["W", "E2"] + G(1, 11), [], True),       # small segments probed: 9 and 12 terms
        (["E0"] + A8, [], True), (G(1, 5) + ["E0"] + G(5, 9), ["X3"], True),        # ... and driving: padding, empty segments
        (["Z1"] + A8, [], True), (["Z0"] + A8, [], True),                           # a term never in field 1; a term without a posting
        (["H1"] + A8, [], True), (["H2"] + A8, ["X4"], True),
        (G(0, 24) + [f"F{i}" for i in range(8)], [], True),                         # 32 terms
        (["W"], [], False), (["E1"], [], False), (["Z1", "G1"], [], False), (["Z0"], [], False),
    ]


def _seam_queries(w):
    """every seam case under every filter, with the route _seam_cases writes beside it"""
    out = []
    for filt in FILTERS:
        for terms, nots, beyond in _seam_cases():
            out.append((w.q(terms, nots, filt), beyond and (w.kind == "P" or bool(filt))))
    return out


def _frequent_queries(w):
    """M: all_terms_frequent with 7 (native) | 8 (gallop) terms, marked at k = 10 (N > 256 k); two term orders"""
    f = [f"F{i}" for i in range(8)]
    return [(w.q(f[:7], freq=True), False), (w.q(f, freq=True), True), (w.q(f[1:], freq=True), False), (w.q(f[::-1], freq=True), True),
            (w.q(f[:2], freq=True), False)]


def _sparse_queries(w):
    """M: filtered intersections and single terms that name a sparse-tier term -- bm25_sparse.hip's gate over the postings' field masks"""
    out = []
    for filt in ((0,), (1, 2)):
        out += [w.q(["S1", "G1"], (), filt), w.q(["S2", "G1", "G2"], (), filt), w.q(["S2"], (), filt), w.q(["S1"], (), filt),
                w.q(["S1", "G1"], ["S3"], filt), w.q(["G1", "G2"], ["S3"], filt), w.q(["S2", "S1"], ["X0"], filt), w.q(["S2", "Z1"], (), filt)]
    return out


# batches by the shares they run at: name -> (queries, the intended P)
def _share_batches(w):
    f = (0,) if w.kind == "M" else ()   # (M: gallop needs a filter)
    g = (1, 2) if w.kind == "M" else ()
    tiny = [w.q(["E0"] + A8, (), f), w.q(["W", "E1"] + G(1, 8), (), g)]
    if w.kind == "M":
        return {
            "tiny drivers": (tiny, 1),                                                    # P = 1: 18 and 40 postings
            "H1": ([w.q(["H1"] + A8, (), f), w.q(A8 + ["H1"], (), g)], 1),                # P = 1: 1 024 <= postings < 2 048
            "H2": ([w.q(["H2"] + A8, (), f), w.q(A8 + ["H2"], ["X4"], g)], 2),            # P = 2
            "G0 and a tiny one": ([w.q(["G0"] + A8, (), f), w.q(A8 + ["G0"], (), g)] + tiny, 3),   # P = 3 (odd); the tiny drivers' shares mostly empty
        }
    return {
        "tiny drivers": (tiny, 1),                                                        # P = 1
        "H1": ([w.q(["H1"] + A8), w.q(A8 + ["H1"], (), (0,))], 2),                        # P = 2: its three field lists hold 2 048 .. 3 071 postings
        "H2": ([w.q(["H2"] + A8), w.q(A8 + ["H2"], ["X4"], (1, 2))], 3),                  # P = 3 (odd)
        "G0 and a tiny one": ([w.q(["G0"] + A8), w.q(A8 + ["G0"], (), (1, 2))] + tiny, 5),   # P = 5 (odd)
    }


def _gallop_shares(w, qs, k=10):
    gq = [x for x in qs if w.gallop(x, k)]
    return _shares(max(w.driver_postings(x) for x in gq), len(gq))


# ---------------------------------------------------------------- P64: 64 shares, and 8192 / nq as the cap
N64 = 6 * 4096 - 5
PAT64 = {5: (0, 1), 11: (1, 2), 21: (0,), 27: (2,)}   # by doc % 32; every other doc holds a term in all three fields


def _build_p64():
    rng = np.random.default_rng(404)
    n = N64
    every = np.arange(n, dtype=np.int64)

    def per_field(docs):
        docs = np.unique(np.asarray(docs, np.int64))
        held = np.ones((len(docs), NF), bool)
        for r, fs in PAT64.items():
            held[docs % 32 == r] = [f in fs for f in range(NF)]
        return [docs[held[:, f]] for f in range(NF)]

    t0 = np.setdiff1d(every, rng.choice(n, int(0.03 * n), replace=False))   # the shortest: it drives
    per0 = per_field(t0)
    special = set()
    for image in _driver_images(per0, False, n):
        for P in (64, 63):
            special |= _share_docs(image, P)
    for r in PAT64:
        special |= set(int(x) for x in t0[t0 % 32 == r][3:6])
    special = np.array(sorted(special), np.int64)
    lists = {"T0": (per0, None)}
    for i in range(1, 10):
        lists[f"T{i}"] = (per_field(np.union1d(special, np.setdiff1d(every, rng.choice(n, int(0.02 * n), replace=False)))), None)
    lists["TT"] = ([np.union1d(special[::40], SEAM[:3])[:19]] * NF, None)   # < 64 postings in all
    cls = rng.choice([0, 1, 3, 4, 5], n)
    cls[special] = TOP
    w = FWorld("P", n, BOOST_P, lists, len(lists), cls, special)
    w.deleted = np.unique(np.concatenate([[0, 63, 64, 4095, 4096, N64 - 1], w.docs("T0")[::3]]))
    return w


def _p64_queries(w):
    t = [f"T{i}" for i in range(10)]
    long_ = [w.q(t[:9]), w.q(t[1:] + ["T0"], (), (0,)), w.q(t[:9], (), (1, 2))]
    tiny = [w.q(["TT"] + t[1:9]), w.q(t[1:9] + ["TT"], (), (0,))]
    return long_, tiny


# ---------------------------------------------------------------- the worlds prove themselves (no GPU)
def test_reference_of_a_world_is_the_oracles():
    """FCorpus.ref (naive.bm25f_exact over the world's entries) against the C oracle on a few of M's queries: the same matches"""
    from oracle import oracle as O
    w = _world("M")
    c = w.c
    for x in (w.q(A8 + ["G9"], (), (0,)), w.q(["W"], NOT10, (1, 2)), w.q(["S2", "G1", "G2"], (), (1, 2)), w.q(["E0"] + A8)):
        ids, sc, rd, rs = w.ref(x, w.deleted)
        od, os_, otot, _ = O.search_fields_exhaustive(c.n_docs, c.doclen, c.boost, c.offs, c.docs, c.fields, c.tfs, list(x.terms), O.OP_AND, c.n_docs,
                                                      not_terms=list(x.nots), deleted=w.deleted, field_filter=x.filt)
        assert otot == len(ids) and np.array_equal(np.sort(od), ids), w.label(x)
        assert np.all(np.abs(os_[np.argsort(od)] - sc) <= REL * sc)


@pytest.mark.parametrize("kind", ["M", "P"])
def test_routes_are_the_seam_table(kind):
    """the restated rule (FWorld.gallop) gives what the seam table says, case by case; every seam has both sides"""
    w = _world(kind)
    seams = _seam_queries(w)
    for x, beyond in seams:
        assert w.gallop(x) == beyond, w.label(x)
    assert {b for _, b in seams} == {True, False}
    if kind == "M":
        for x, beyond in _frequent_queries(w):
            assert w.gallop(x, 10) == beyond and not w.gallop(x, 129), w.label(x)
        assert not any(w.gallop(x) for x in _sparse_queries(w))
        assert not any(w.gallop(x) for x, _ in seams if not x.filt)   # (no filter: the merged lists, one list per term)
    else:
        assert all(w.gallop(x) == b for x, b in seams)
    n_lists = {(len(x.terms) + len(x.nots)) * NF for x, _ in seams}
    assert {24, 27, 30, 33} <= n_lists and max(n_lists) == 96


@pytest.mark.parametrize("kind", ["M", "P"])
def test_world_holds_what_it_is_built_for(kind):
    w = _world(kind)
    n = N_DOCS
    # segments of 0, 4 and 5 postings in (term, field) lists, probed at local docs 0 and 4095 and one past the last posting by W
    probe, seen = w.docs("W"), set()
    for name, fl in E_SEGS.items():
        for f, segs in enumerate(fl):
            if segs == "bulk":
                assert 300 <= len(w.per_field[name][f]) <= 303 and np.isin(BULK_W, w.per_field[name][f]).all()
                continue
            d = w.per_field[name][f]
            assert np.array_equal(d, _seg_docs(segs))
            for sb in range(4):
                seg = d[(d >> 12) == sb]
                seen.add(len(seg))
                hi = min(sb * 4096 + 4095, n - 1)
                assert sb * 4096 in probe and hi in probe
                if len(seg) and seg[-1] < hi:
                    assert seg[-1] + 1 in probe and seg[-1] + 1 not in seg
    assert {0, 4, 5} <= seen
    assert len(w.per_field["E1"][1]) == 0 and len(w.docs("Z0")) == 0                   # an empty field list; a term with no posting
    assert len(w.per_field["Z1"][1]) == 0 and min(len(w.per_field["Z1"][f]) for f in (0, 2)) > 100
    for name in G(0, 13):                                                              # 25 - 50 % of the docs, the seam docs in every one
        assert 0.25 <= len(w.docs(name)) / n <= 0.5 and np.isin(SEAM, w.docs(name)).all()
        per = w.per_field[name]                                                        # all three fields / the last only / the first only
        assert np.isin(per[0], per[1]).any() and not np.isin(per[2], per[0]).all() and not np.isin(per[0], per[2]).all()
    sizes = {name: _driver_postings(w.per_field[name], w.merged) for name in G(0, 24) + [f"F{i}" for i in range(8)]}
    assert all(sizes["G0"] < v for k_, v in sizes.items() if k_ != "G0")              # G0 strictly the shortest wide list
    for i in range(8):
        assert len(w.docs(f"F{i}")) >= n / 2
    size = lambda name: _driver_postings(w.per_field[name], w.merged)
    assert size("W") < min(size("E1"), size("E2"), sizes["G0"]) and size("E0") < sizes["G0"]   # W drives E1 / E2 (they are probed); E0 drives
    assert np.isin(TOMB, w.deleted).all() and np.isin(w.docs("G0")[::3], w.deleted).all()
    if kind == "M":
        assert w.names[w.nd:] == ["S1", "S2", "S3"] and len(w.per_field["S2"][1]) == 0
    # every seam query (but the one naming Z0) has matches, with and without tombstones; the filters really remove docs
    removed = 0
    for x, beyond in _seam_queries(w):
        for deleted in ((), w.deleted):
            total = len(w.ref(x, deleted)[0])
            assert (total > 0) != (w.id["Z0"] in x.terms), w.label(x)
        if x.filt:
            removed += len(w.ref(x._replace(filt=()))[0]) - len(w.ref(x)[0])
    assert removed > 1000
    wide = [len(w.ref(w.q(t, (), f))[0]) for f in FILTERS for t in (A8 + ["G9"], G(0, 12), G(0, 24) + [f"F{i}" for i in range(8)])]
    assert min(wide) > 257, wide                                                       # intersections of 9, 12 and 32 terms: beyond k = 257
    if kind == "M":
        for x, beyond in _frequent_queries(w):                                         # the rule ranks some docs, not all, and changes the top 10
            ids, sc, rd, rs = w.ref(x, (), True)
            all_ids, _, all_rd, _ = w.ref(x)
            assert 10 < len(ids) < len(all_ids) and not np.array_equal(rd[:10], all_rd[:10]), w.label(x)
        for x in _sparse_queries(w):
            assert len(w.ref(x)[0]) > 0 and len(w.ref(x)[0]) < len(w.ref(x._replace(filt=()))[0]), w.label(x)


@pytest.mark.parametrize("kind", ["M", "P"])
def test_shares_and_their_seam_docs(kind):
    """every share batch runs at the P written beside it (1, 2, an odd one among them); the docs in the first and last slot of every
    share of its long driver, those next to NULL padding and some the driver holds in two field lists match the query and rank:
    every one (P: that holds field 0) within the reference's top 1024, those that hold all three fields within its top 128"""
    w = _world(kind)
    seen = set()
    for name, (qs, intended) in _share_batches(w).items():
        assert all(w.gallop(x) for x in qs), name
        P = _gallop_shares(w, qs)
        assert P == intended, (kind, name, P, [w.driver_postings(x) for x in qs])
        seen.add(P)
        if name == "tiny drivers":
            continue
        for x in qs[:2]:
            drv = min(x.terms, key=lambda t: _driver_postings(w.per_field[w.names[t]], w.merged))
            must = set()
            for image in _driver_images(w.per_field[w.names[drv]], w.merged, N_DOCS):
                assert (image < 0).any()
                must |= _share_docs(image, P)
            assert must <= set(w.special.tolist()) and len(must) >= 2 * P
            per = w.per_field[w.names[drv]]
            assert np.isin(w.special, np.intersect1d(per[0], per[1])).any()   # held in two field lists of the driver
            for deleted in ((), w.deleted):
                ids, sc, rd, rs = w.ref(x, deleted)
                m = np.array(sorted(must & set(ids.tolist())), np.int64)
                assert len(m) >= (0 if len(deleted) else P), (name, len(m))   # (tombstones stand on some of them)
                best = m[m % 4 == 0]   # (all three fields and the top weight class: only other such docs tie with them)
                high = m if w.merged else m[np.isin(m % 4, (0, 2))]   # (P: field 0 carries the score, boost 4096)
                assert np.isin(high, rd[:1024]).all() and np.isin(best, rd[:128]).all() and (len(best) or len(deleted)), w.label(x)
    assert {1, 2} <= seen and any(p > 1 and p % 2 for p in seen)


def test_p64_world_runs_at_64_shares_and_under_the_cap():
    w = _world("P64")
    assert w.c.n_docs == N64 and (N64 + 4095) // 4096 == 6 and not w.merged
    long_, tiny = _p64_queries(w)
    assert all(w.gallop(x) for x in long_ + tiny)
    assert w.driver_postings(long_[0]) >= 65536 and all(w.driver_postings(x) < 64 for x in tiny)
    assert _gallop_shares(w, long_ + tiny) == 64                               # P = 64
    assert _gallop_shares(w, long_[:1] + tiny * 64) == 63                      # 129 queries: 8192 / nq = 63 is the cap (an odd P again)
    per = w.per_field["T0"]
    assert all(len(np.setdiff1d(np.intersect1d(per[a], per[b]), per[c])) for a, b, c in ((0, 1, 2), (1, 2, 0)))   # docs in two field lists only
    for x in long_:
        ids, sc, rd, rs = w.ref(x)
        must = set()
        for image in _driver_images(per, False, N64):
            must |= _share_docs(image, 64) | _share_docs(image, 63)
        assert must <= set(w.special.tolist())
        m = np.array(sorted(must & set(ids.tolist())))
        ranked = m[np.isin(m, per[0])]     # (field 0 carries the score: boost 4096)
        assert len(ranked) > 200 and np.isin(ranked, rd[:1024]).all(), (w.label(x), len(ranked))
    chunks = (len(_padded(w.per_field["TT"][0], N64)) + 63) >> 6
    assert chunks == 1 and [((chunks * p) // 64) << 6 for p in range(65)].count(0) == 64   # a tiny driver: 63 of its 64 shares are empty


@pytest.mark.parametrize("kind", ["M", "P", "P64"])
def test_exact_ties_are_proven_for_enough_queries(kind):
    """where FWorld.exact holds the GPU tests ask for the reference's very list; it must hold for gallop queries of every kind"""
    w = _world(kind)
    if kind == "P64":
        long_, tiny = _p64_queries(w)
        qs = long_ + tiny
    else:
        qs = [x for x, _ in _seam_queries(w)] + (_sparse_queries(w) if kind == "M" else [])
    exact = [x for x in qs if w.exact(x, w.deleted) and len(w.ref(x, w.deleted)[0]) > 1]
    tied = [x for x in exact if len(np.unique(w.ref(x, w.deleted)[3])) < len(w.ref(x, w.deleted)[3])]
    print(f"world {kind}: exact ties proven for {len(exact)} of {len(qs)} queries, {sum(w.gallop(x) for x in exact)} of them gallop queries, "
          f"{len(tied)} with tied scores")
    assert sum(w.gallop(x) for x in tied) >= (2 if kind == "P64" else 3), kind   # (P64: the two queries a tiny list drives)
    if kind == "M":
        fr = [x for x, _ in _frequent_queries(w) if w.exact(x, (), True)]
        print(f"  all_terms_frequent: {len(fr)} of 5")


_RT = types.SimpleNamespace(ResultType=types.SimpleNamespace(Topk="topk", TopkCount="topkcount", Count="count"))


def test_the_checks_reject_altered_answers():
    """_check on hand-altered answers of P's [G0, G1 .. G8] at k = 10: a doc twice; a doc answered under a partial score -- what its
    field-0 entries alone give, as a kernel would that met it in one field list; a tie group whose docs come back in the order of the
    field lists a driver walks (higher ids first); a tied doc replaced by a later one of its group.  The unaltered answer passes"""
    w = _world("P")
    x = w.q(["G0"] + A8)
    k = 10
    assert w.exact(x)
    ids, sc, rd, rs = w.ref(x)
    view = w.c.view(x.filt)

    def check(d, s):
        d, s = np.asarray(d, np.uint32), np.asarray(s, np.float32)
        _check(view, "altered", x.terms, x.op_and, x.nots, (), k, _RT.ResultType.TopkCount, d, s, len(d), len(ids), _RT, exact_ties=True)

    good_d, good_s = rd[:k].copy(), rs[:k].astype(np.float32)
    check(good_d, good_s)
    d = good_d.copy()
    d[5] = d[4]
    with pytest.raises(AssertionError, match="a doc twice"):
        check(d, good_s)
    # the top doc under the score of its field-0 entries alone (boost 4096 beside 1 and 1 / 4096: 2.4e-4 and more below the full score)
    c = w.c
    comp = naive.component_cache(np.float32(int(naive.DLC[c.doclen].astype(np.uint64).sum())) / np.float32(c.n_docs))
    partial = 0.0
    for t in x.terms:
        dd, ff, tf = c.entries[t]
        i = np.nonzero((dd == rd[0]) & (ff == 0))[0]
        assert len(i) == 1 and np.any((dd == rd[0]) & (ff == 1))   # (the doc holds the term in field 1 as well)
        tf32 = np.float32(tf[i[0]])
        partial += float(c.boost[0]) * float(naive.idf(c.n_docs, len(np.unique(dd)))) * float((tf32 * np.float32(2.2)) / (tf32 + comp[c.doclen[0, rd[0]]]))
    assert partial < rs[0] * (1 - REL)
    with pytest.raises(AssertionError, match="scored"):
        check(good_d, np.append(np.float32(partial), good_s[1:]))
    tie = np.nonzero(good_s == good_s[-1])[0]
    assert len(tie) >= 2 and rs[k] == rs[k - 1]   # the tie group straddles rank k
    d = good_d.copy()
    d[tie] = d[tie][::-1]
    with pytest.raises(AssertionError, match="out of doc-id order"):
        check(d, good_s)
    d = good_d.copy()
    d[tie[-1]] = rd[k]
    with pytest.raises(AssertionError, match="lowest doc ids first"):
        check(d, good_s)


# ---------------------------------------------------------------- the GPU
@pytest.fixture(scope="module")
def S():
    import seekstorm_amd
    return seekstorm_amd


@pytest.fixture(scope="module")
def N():
    from seekstorm_amd import _native
    return _native


def _upload(S, w):
    c = w.c
    e = int(c.offs[w.nd])
    sh = S.Shard(0)
    sh.upload_lexical_fields(c.n_docs, c.doclen, c.boost, c.offs[:w.nd + 1], c.docs[:e], c.fields[:e], c.tfs[:e])
    if w.merged:
        assert sh.fields_info()[1]
        assert sh.append_sparse_fields(c.offs[w.nd:] - c.offs[w.nd], c.docs[e:], c.fields[e:], c.tfs[e:]) == w.nd
        assert sh.sparse_info()[0] == len(w.names) - w.nd
    else:
        assert sh.fields_info()[:2] == (3, False)
    assert [int(v) for v in sh.posting_count(np.arange(len(w.names)))] == [len(w.docs(name)) for name in w.names]
    w.rows = {}
    return sh


@pytest.fixture(scope="module")
def shard_m(S):
    sh = _upload(S, _world("M"))
    yield sh
    sh.close()


@pytest.fixture(scope="module")
def shard_p(S):
    sh = _upload(S, _world("P"))
    yield sh
    sh.close()


@pytest.fixture(scope="module")
def shard_p64(S):
    sh = _upload(S, _world("P64"))
    yield sh
    sh.close()


def _rows(S, sh, w, qs, k):
    """the queries as one batch (make_queries takes one filter per call: a row each, cached); all_terms_frequent marked at k = 10"""
    out = []
    for x in qs:
        key = (x, x.freq and k == 10)
        if key not in w.rows:
            q = sh.make_queries([list(x.terms)], S.QueryType.Intersection if x.op_and else S.QueryType.Union, [list(x.nots)], field_filter=x.filt)
            if key[1]:
                q = sh.mark_all_terms_frequent(q, k)
                assert q["op"][0] >> 31, w.label(x)
            w.rows[key] = q
        out.append(w.rows[key])
    return np.concatenate(out)


def _search(S, sh, w, qs, k, rt, deleted, what, facet_filter=None):
    """one call; every row against the reference; -> the sub-batches the galloping kernel answered"""
    q = _rows(S, sh, w, qs, k)
    before = sh.generic_batches()
    d, s, cnt, tot = sh.search_lexical_batch(q, k, rt, reference_shortcuts=False, facet_filter=facet_filter)
    gen = sh.generic_batches() - before
    for j, x in enumerate(qs):
        where = f"{what} row {j} k={k} rt={int(rt)} {w.label(x)}"
        freq = x.freq and k == 10
        exact = w.exact(x, deleted, freq)
        view = w.c.view(x.filt, freq)
        if freq:   # every match counted, the docs the rule ranks returned
            if rt != S.ResultType.Topk:
                assert int(tot[j]) == len(w.ref(x, deleted)[0]), f"{where}: result_count_total {int(tot[j])}"
            if rt != S.ResultType.Count:
                _check(view, where, x.terms, x.op_and, x.nots, deleted, k, S.ResultType.Topk, d[j], s[j], cnt[j], tot[j], S, exact)
        else:
            _check(view, where, x.terms, x.op_and, x.nots, deleted, k, rt, d[j], s[j], cnt[j], tot[j], S, exact)
    want = int(any(w.gallop(x, k) for x in qs))
    # (a page beyond SS_MAX_K is answered in passes, each a call of its own)
    assert gen == want or (k > 1024 and want and gen > want), f"{what} k={k} rt={int(rt)}: {gen} generic sub-batches"
    return gen


def _every_k(S, sh, w, qs, deleted, what, ks=KS):
    for k in ks:
        for rt in (S.ResultType.Topk, S.ResultType.TopkCount, S.ResultType.Count):
            if rt == S.ResultType.Count and k != 10:
                continue
            _search(S, sh, w, qs, k, rt, deleted, what)


def _shard_of(kind, shard_m, shard_p):
    return shard_m if kind == "M" else shard_p


@pytest.mark.gpu
@pytest.mark.parametrize("tombstones", [False, True])
@pytest.mark.parametrize("kind", ["M", "P"])
def test_routing_seams(S, N, shard_m, shard_p, kind, tombstones):
    """every seam query alone (its side of the seam by the counter), then all of them in one call at every k and result type"""
    w, sh = _world(kind), _shard_of(kind, shard_m, shard_p)
    deleted = w.deleted if tombstones else ()
    sh.set_deleted(deleted)
    try:
        seams = _seam_queries(w)
        for x, beyond in seams:
            assert _search(S, sh, w, [x], 10, S.ResultType.TopkCount, deleted, "alone") == int(beyond), w.label(x)
        _every_k(S, sh, w, [x for x, _ in seams], deleted, "seams")
        if not tombstones:
            _search(S, sh, w, [x for x, _ in seams], K_DEEP, S.ResultType.TopkCount, deleted, "deep page")
    finally:
        sh.set_deleted([])


@pytest.mark.gpu
@pytest.mark.parametrize("tombstones", [False, True])
def test_all_terms_frequent_seam(S, N, shard_m, tombstones):
    """M: 7 | 8 terms of lists in more than half of the docs, tf 9 | 10 in the lowest field: the mark read from a merged code"""
    w, sh = _world("M"), shard_m
    deleted = w.deleted if tombstones else ()
    sh.set_deleted(deleted)
    try:
        fq = _frequent_queries(w)
        for x, beyond in fq:
            assert _search(S, sh, w, [x], 10, S.ResultType.TopkCount, deleted, "alone") == int(beyond), w.label(x)
        for rt in (S.ResultType.Topk, S.ResultType.TopkCount, S.ResultType.Count):
            _search(S, sh, w, [x for x, _ in fq], 10, rt, deleted, "frequent")
    finally:
        sh.set_deleted([])


@pytest.mark.gpu
@pytest.mark.parametrize("tombstones", [False, True])
def test_sparse_terms_under_a_filter_take_the_gate(S, N, shard_m, tombstones):
    """M: filtered intersections and single terms naming a sparse-tier term (one that passes only through its last field, a sparse NOT
    term): bm25_sparse.hip's gate over the field masks of the postings -- the counter of the galloping kernel stays"""
    w, sh = _world("M"), shard_m
    deleted = w.deleted if tombstones else ()
    sh.set_deleted(deleted)
    try:
        qs = _sparse_queries(w)
        for x in qs:
            assert _search(S, sh, w, [x], 10, S.ResultType.TopkCount, deleted, "alone") == 0
        _every_k(S, sh, w, qs, deleted, "sparse gate", ks=(1, 10, 129, 1024))
    finally:
        sh.set_deleted([])


@pytest.mark.gpu
@pytest.mark.parametrize("tombstones", [False, True])
@pytest.mark.parametrize("kind", ["M", "P"])
def test_share_batches(S, N, shard_m, shard_p, kind, tombstones):
    """batches at P = 1, 2 and odd Ps: the share seams of a long driver, a tiny driver beside it"""
    w, sh = _world(kind), _shard_of(kind, shard_m, shard_p)
    deleted = w.deleted if tombstones else ()
    sh.set_deleted(deleted)
    try:
        for name, (qs, intended) in _share_batches(w).items():
            assert _gallop_shares(w, qs) == intended
            _every_k(S, sh, w, qs, deleted, f"shares {name} (P = {intended})")
    finally:
        sh.set_deleted([])


@pytest.mark.gpu
@pytest.mark.parametrize("tombstones", [False, True])
def test_64_shares_and_the_cap(S, N, shard_p64, tombstones):
    """P64: the long drivers at P = 64 beside tiny ones (63 of their 64 shares empty), then 129 queries: 8192 / nq = 63 caps P"""
    w, sh = _world("P64"), shard_p64
    deleted = w.deleted if tombstones else ()
    sh.set_deleted(deleted)
    try:
        long_, tiny = _p64_queries(w)
        assert _gallop_shares(w, long_ + tiny) == 64
        for k, rt in ((10, S.ResultType.TopkCount), (1024, S.ResultType.TopkCount), (1024, S.ResultType.Topk), (10, S.ResultType.Count)):
            _search(S, sh, w, long_ + tiny, k, rt, deleted, "P = 64")
        capped = long_[:1] + tiny * 64
        assert _gallop_shares(w, capped) == 63
        _search(S, sh, w, capped, 257, S.ResultType.TopkCount, deleted, "P = 63, capped by 8192 / nq")
    finally:
        sh.set_deleted([])


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["M", "P"])
def test_one_shuffled_call(S, N, shard_m, shard_p, kind):
    """everything in ONE shuffled call: the library splits it per kernel family and must answer in the caller's order"""
    w, sh = _world(kind), _shard_of(kind, shard_m, shard_p)
    qs = [x for x, _ in _seam_queries(w)]
    if kind == "M":
        qs += [x for x, _ in _frequent_queries(w)] + _sparse_queries(w)
    for _, (sq, _p) in _share_batches(w).items():
        qs += sq
    qs = [qs[i] for i in np.random.default_rng(7).permutation(len(qs))]
    try:
        for deleted in ((), w.deleted):
            sh.set_deleted(deleted)
            for k, rt in ((10, S.ResultType.TopkCount), (10, S.ResultType.Topk), (10, S.ResultType.Count), (129, S.ResultType.TopkCount)):
                _search(S, sh, w, qs, k, rt, deleted, "shuffled")
    finally:
        sh.set_deleted([])


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["M", "P"])
def test_gallop_under_a_facet_filter(S, N, shard_m, shard_p, kind):
    """a one-range numeric facet filter with NO tombstones set: the exclusion bitmap is swapped in with deleted_words taken from the
    facet records; the last doc is filtered out.  The reference: the filtered docs passed as tombstones"""
    w, sh = _world(kind), _shard_of(kind, shard_m, shard_p)
    val = (np.arange(N_DOCS) % 251).astype(np.uint8)
    val[-1] = 255
    sh.upload_facets(val.reshape(N_DOCS, 1))
    sh.set_deleted([])
    out = np.nonzero(~((val >= 5) & (val < 250)))[0]
    assert out[-1] == N_DOCS - 1
    x = w.q(["G0"] + A8, ["X0"], (0,))
    assert w.gallop(x)
    for k in (10, 129):
        for rt in (S.ResultType.TopkCount, S.ResultType.Topk, S.ResultType.Count):
            assert _search(S, sh, w, [x], k, rt, out, "facet filter", facet_filter=[(0, "u8", 5, 250)]) == 1


# ---------------------------------------------------------------- "bit-identical to the specialised kernels where both can answer"
PHRASES = ([18, 19], [20, 21, 22], [18, 19, 20, 21, 22, 23], [23, 18, 19, 20])   # 2 .. 6 unique terms, planted in > 129 docs each


def _text_world(n_fields, seed):
    """docs as texts (per field) over 24 terms: terms 0 .. 17 at random, the phrases planted over terms 18 .. 23 (short lists), near
    misses with the words reversed -- as _phrase_corpus of test_gpu_score_edges builds them; -> upload arrays, positions, the texts"""
    rng = np.random.default_rng(seed)
    n, width = 2 * 4096 + 1, 40
    lens = rng.integers(20, width + 1, (n_fields, n))
    texts = rng.integers(0, 18, (n_fields, n, width))
    texts[np.arange(width)[None, None, :] >= lens[:, :, None]] = -1
    for i, ph in enumerate(PHRASES):
        for d in range(300 * i, 300 * i + 450):   # (ranges overlap: docs holding two of the phrases)
            f = d % n_fields
            at = int(rng.integers(0, lens[f, d] - len(ph) + 1))
            texts[f, d, at:at + len(ph)] = ph if d % 9 else ph[::-1]
    f_, d_, p_ = np.nonzero(texts >= 0)
    t_ = texts[f_, d_, p_]
    o = np.lexsort((p_, f_, d_, t_))
    f_, d_, p_, t_ = f_[o], d_[o], p_[o], t_[o]
    new = np.ones(len(t_), bool)
    new[1:] = (t_[1:] != t_[:-1]) | (d_[1:] != d_[:-1]) | (f_[1:] != f_[:-1])
    start = np.nonzero(new)[0]
    tfs = np.diff(np.append(start, len(t_))).astype(np.uint16)
    docs, fields, terms = d_[start].astype(np.uint32), f_[start].astype(np.uint8), t_[start]
    offs = np.searchsorted(terms, np.arange(25)).astype(np.uint64)
    dl = np.array([[_b4(x) for x in row] for row in lens], np.uint8)
    return n, dl, offs, docs, fields, tfs, p_.astype(np.uint16), texts


def _phrase_matches(texts, ph):
    """brute force: the docs where the words of ph stand side by side inside one field"""
    width = texts.shape[2] - len(ph) + 1
    m = np.ones(texts.shape[:2] + (width,), bool)
    for i, t in enumerate(ph):
        m &= texts[:, :, i:i + width] == t
    return np.nonzero(m.any(axis=(0, 2)))[0]


def test_text_worlds_hold_their_phrases():
    for n_fields in (1, 3):
        n, dl, offs, docs, fields, tfs, pos, texts = _text_world(n_fields, 61 + n_fields)
        assert len(pos) == int(tfs.astype(np.int64).sum())
        df = np.diff(offs.astype(np.int64))
        assert df[18:].max() < df[:18].min()   # the phrase terms' lists are the shortest
        for ph in PHRASES:
            assert 129 < len(_phrase_matches(texts, ph)) < n // 4, ph


def _phrase_native_vs_gallop(S, sh, texts):
    q = sh.make_queries([list(p) for p in PHRASES], S.QueryType.Phrase)
    before = sh.generic_batches()
    d0, s0, c0, t0 = sh.search_lexical_batch(q, 128, S.ResultType.TopkCount)
    assert sh.generic_batches() == before       # <= 6 unique terms, k <= 128: the phrase kernels of the probe index
    d1, s1, c1, t1 = sh.search_lexical_batch(q, 129, S.ResultType.TopkCount)
    assert sh.generic_batches() == before + 1   # k = 129: the galloping kernel
    assert np.array_equal(d0, d1[:, :128]) and np.array_equal(s0, s1[:, :128]) and np.array_equal(t0, t1)
    assert np.all(c0 == 128) and np.all(c1 == 129)
    for i, ph in enumerate(PHRASES):
        m = _phrase_matches(texts, ph)
        assert int(t1[i]) == len(m) and np.isin(d1[i], m).all() and len(np.unique(d1[i])) == 129, ph


@pytest.mark.gpu
def test_phrase_native_and_gallop_one_field(S, N):
    n, dl, offs, docs, fields, tfs, pos, texts = _text_world(1, 62)
    sh = S.Shard(0)
    try:
        sh.upload_lexical(n, dl[0], offs, docs, tfs, positions=pos)
        _phrase_native_vs_gallop(S, sh, texts)
    finally:
        sh.close()


@pytest.mark.gpu
def test_phrase_native_and_gallop_three_fields(S, N):
    """M's fields and boosts over texts: merged lists with field-tagged positions"""
    n, dl, offs, docs, fields, tfs, pos, texts = _text_world(3, 64)
    sh = S.Shard(0)
    try:
        sh.upload_lexical_fields(n, dl, BOOST_M, offs, docs, fields, tfs, positions=pos)
        assert sh.fields_info() == (3, True, True)
        _phrase_native_vs_gallop(S, sh, texts)
    finally:
        sh.close()


@pytest.mark.gpu
def test_phrase_on_rowless_lists_equals_the_full_shard(S, N):
    """rationed probe rows (12 for 24 lists, the longest first): the phrase terms' lists stay row-less and their phrases take the
    galloping kernel; the full shard answers them with the probe index's phrase kernel -- the same rows, bit for bit"""
    n, dl, offs, docs, fields, tfs, pos, texts = _text_world(1, 62)
    full, part = S.Shard(0), S.Shard(0)
    try:
        full.upload_lexical(n, dl[0], offs, docs, tfs, positions=pos)
        part.set_probe_budget((12 + 1) * ((n + 4095) // 4096) * 64 * 12)
        part.upload_lexical(n, dl[0], offs, docs, tfs, positions=pos)
        assert not part.terms_probed(list(range(18, 24))).any() and full.terms_probed(list(range(24))).all()
        for k in (10, 100):
            gf, gp = full.generic_batches(), part.generic_batches()
            a = full.search_lexical_batch(full.make_queries([list(p) for p in PHRASES], S.QueryType.Phrase), k)
            b = part.search_lexical_batch(part.make_queries([list(p) for p in PHRASES], S.QueryType.Phrase), k)
            assert full.generic_batches() == gf and part.generic_batches() == gp + 1
            assert all(np.array_equal(u, v) for u, v in zip(a, b)), k
            for i, ph in enumerate(PHRASES):
                assert int(a[3][i]) == len(_phrase_matches(texts, ph))
    finally:
        full.close()
        part.close()


def _frequent_world():
    """one indexed field: L0 .. L6 in 55 - 70 % of the docs, tf 9 where doc % 11 names the list (the rule leaves those docs unranked),
    else 10 .. 13; L7 holds every doc with tf 10"""
    rng = np.random.default_rng(505)
    n = N_DOCS
    cls = rng.integers(0, 2, n)
    dl = np.array([_b4(8), _b4(300)], np.uint8)[cls][None, :]
    ent = []
    for t in range(7):
        d = np.union1d(SEAM, rng.choice(n, int((0.55 + 0.025 * t) * n), replace=False)).astype(np.int64)
        ent.append((d, np.zeros(len(d), np.int64), np.where(d % 11 == t, 9, 10 + (d * 3 + t) % 4)))
    every = np.arange(n, dtype=np.int64)
    ent.append((every, np.zeros(n, np.int64), np.full(n, 10)))
    return FCorpus(n, dl, [1.0], ent)


def test_frequent_world_ranks_some_docs():
    c = _frequent_world()
    ids, sc, rd, rs = c.ref(list(range(7)), True, frequent=True)
    all_ids = c.ref(list(range(7)), True)[0]
    assert 129 < len(ids) < len(all_ids)
    assert np.array_equal(c.ref(list(range(8)), True, frequent=True)[0], ids)   # L7 holds every doc with tf 10: the same docs ranked
    assert np.float32(1e-30) > 0 and np.float32(np.float32(1e-30) * np.float32(4.0)) < np.spacing(np.float32(rs.min())) / 4   # fmaf(1e-30, w, s) == s


@pytest.mark.gpu
@pytest.mark.parametrize("tombstones", [False, True])
def test_frequent_native_and_gallop_one_field(S, N, tombstones):
    """7 terms: the specialised kernels; the same 7 and L7 (every doc, tf 10) under an idf of 1e-30: the galloping kernel, whose
    chain ends in fmaf(1e-30, w, s) == s -- docs, scores, counts and totals equal bit for bit; the 7-term answer against the reference"""
    c = _frequent_world()
    deleted = np.unique(np.concatenate([TOMB, c.entries[0][0][::3]])) if tombstones else np.zeros(0, np.int64)
    sh = S.Shard(0)
    try:
        sh.upload_lexical(c.n_docs, c.doclen[0], c.offs, c.docs, c.tfs)
        sh.set_deleted(deleted)
        for order in (list(range(7)), [3, 6, 0, 5, 1, 4, 2]):
            q7 = sh.mark_all_terms_frequent(sh.make_queries([order], S.QueryType.Intersection), 10)
            q8 = sh.mark_all_terms_frequent(sh.make_queries([order + [7]], S.QueryType.Intersection, idf_of={7: 1e-30}), 10)
            assert q7["op"][0] >> 31 and q8["op"][0] >> 31
            for rt in (S.ResultType.TopkCount, S.ResultType.Topk):
                before = sh.generic_batches()
                a = sh.search_lexical_batch(q7, 10, rt, reference_shortcuts=False)
                assert sh.generic_batches() == before
                b = sh.search_lexical_batch(q8, 10, rt, reference_shortcuts=False)
                assert sh.generic_batches() == before + 1
                assert all(np.array_equal(u, v) for u, v in zip(a, b)), (order, rt)
                _check(c.view((), True), f"frequent {order}", order, True, (), deleted, 10, S.ResultType.Topk, a[0][0], a[1][0], a[2][0], a[3][0], S)
                if rt == S.ResultType.TopkCount:
                    assert int(a[3][0]) == len(c.ref(order, True, (), deleted)[0])
    finally:
        sh.close()
