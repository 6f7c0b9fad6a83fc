"""Return codes of the entries that upload a BM25 image or commit to one, for bad inputs alone and in pairs, and what a refusal leaves
behind (csrc/api_image.hip; -m gpu).

ss_bm25_upload[_positions], ss_bm25_upload_fields[_positions], ss_bm25_append_level[_positions], ss_bm25_append_level_fields,
ss_bm25_append_sparse_level and the four ss_bm25_append_sparse* check their arguments, the shard's state and the postings in an order
that is part of their behaviour: which refusal wins when two apply, and whether the image the shard held survives.  One table of rows
(ROWS), every row an override of an entry's valid call; every row alone and every pair of rows goes to every entry the rows apply to,
and the code is compared with a literal.  The literals (CODES) are the codes commit 5f760f3 returns: read off the order of its checks
first, then confirmed by running this test against a build of that commit.  No row or pair is accepted by the library, every refusal
comes from a host-side check, and every array stays as long as the largest offset handed over says.

The world: 65 536 + 4 099 docs (a full level and a partial one that ends three docs behind a 4 096-doc sub-block), 5 terms, once with
one indexed field and once with two; 4 rare lists over the docs of the second level.  Shards: `main` / `mainp` (the two levels
committed without / with positions), `mainf` (two fields, committed), `tiered` (main + the rare lists as a tier of levels), `tieredf`
(mainf + the rare lists as whole sparse lists), `whole` / `wholef` (uploaded in one call), `empty`, and `scratch`, which the four
whole-image uploads write to.

An upload's letter is upper case where the image `scratch` held before the call is still there afterwards (ss_bm25_info: SS_OK) and
lower case where it is gone (SS_ESTATE): a re-upload refused by the entry's own argument checks keeps the old image, one refused
while the new image is built has already released it.

A commit (ss_bm25_append_level*) that is refused changes nothing: levels, ss_bm25_info and the answers of unions and intersections
under both strategies are what they were, bit for bit."""

import numpy as np
import pytest

from test_gpu_commit import _level_slices
from test_gpu_parity import _fields_corpus

pytestmark = pytest.mark.gpu

FULL, PART = 65536, 4099
N_DOCS = FULL + PART
VOC = [1500, 2500, 3300, 3800, 4050]
DFS = [21_000, 9_000, 3_000, 700, 90]
BOOST = np.array([2.0, 1.0], np.float32)
QUERIES = [[4, 3], [4, 2, 1], [0, 4], [3, 2], [1]]
K = 10
LETTER = {0: "K", -1: "I", -2: "M", -3: "D", -4: "N", -5: "S"}  # OK, EINVAL, ENOMEM, EDEVICE, ENOTSUP, ESTATE

UPLOADS = ("upload", "upload_positions", "upload_fields", "upload_fields_positions")
LEVELS = ("append_level", "append_level_positions", "append_level_fields")
SPARSE = ("append_sparse", "append_sparse_fields", "append_sparse_positions", "append_sparse_fields_positions")
# the C entry and its parameters in order (n_terms: n_lists of the sparse entries)
ENTRY = {
    "upload": ("ss_bm25_upload", "shard n_docs doclen n_terms offs docs tfs"),
    "upload_positions": ("ss_bm25_upload_positions", "shard n_docs doclen n_terms offs docs tfs positions n_positions"),
    "upload_fields": ("ss_bm25_upload_fields", "shard n_docs n_fields doclen boost n_terms offs docs fields tfs"),
    "upload_fields_positions": ("ss_bm25_upload_fields_positions", "shard n_docs n_fields doclen boost n_terms offs docs fields tfs positions n_positions"),
    "append_level": ("ss_bm25_append_level", "shard level n_level_docs doclen n_terms offs docs tfs"),
    "append_level_positions": ("ss_bm25_append_level_positions", "shard level n_level_docs doclen n_terms offs docs tfs npos positions n_positions"),
    "append_level_fields": ("ss_bm25_append_level_fields", "shard level n_level_docs n_fields doclen boost n_terms offs docs fields tfs"),
    "append_sparse_level": ("ss_bm25_append_sparse_level", "shard level n_terms offs docs tfs npos positions n_positions"),
    "append_sparse": ("ss_bm25_append_sparse", "shard n_terms offs docs tfs first"),
    "append_sparse_fields": ("ss_bm25_append_sparse_fields", "shard n_terms offs docs fields tfs first"),
    "append_sparse_positions": ("ss_bm25_append_sparse_positions", "shard n_terms offs docs tfs positions n_positions npos first"),
    "append_sparse_fields_positions": ("ss_bm25_append_sparse_fields_positions", "shard n_terms offs docs fields tfs positions n_positions npos first"),
}
PARAMS = {e: set(p.split()) for e, (_, p) in ENTRY.items()}


def _changed(a, key, at, value):
    x = a[key].copy()
    x[at] = value
    return x


def _swapped(a):
    x = a["docs"].copy()
    j = a["swap_at"]
    x[j], x[j + 1] = x[j + 1], x[j]
    return x


def _repeated(a):
    """the second position of the first posting of term 3 (tf >= 2) repeats the first"""
    o = a["offs"]
    at = int(a["tfs"][int(o[0]):int(o[3])].astype(np.int64).sum())
    return _changed(a, "positions_all", at + 1, a["positions_all"][at])


def _one_more_term(a):
    return np.concatenate([a["offs"], a["offs"][-1:]])


# (name, the entries it goes to -- a set of names, or the parameters an entry must take --, the overrides as functions of the valid call)
ROWS = [
    ("null shard", set(), {"shard": lambda a: None}),
    ("null offs", set(), {"offs": lambda a: None}),
    ("null docs", set(), {"docs": lambda a: None}),
    ("null tfs", set(), {"tfs": lambda a: None}),
    ("null fields", {"fields"}, {"fields": lambda a: None}),
    ("n_terms = 0", set(ENTRY) - set(SPARSE), {"n_terms": lambda a: 0}),  # (no lists are nothing to append: SS_OK)
    ("n_docs = 0", {"n_docs"}, {"n_docs": lambda a: 0}),
    ("n_level_docs = 0", {"n_level_docs"}, {"n_level_docs": lambda a: 0}),
    ("n_level_docs = 65537", {"n_level_docs"}, {"n_level_docs": lambda a: 65537}),
    ("decreasing offs", set(), {"offs": lambda a: _changed(a, "offs", 2, a["offs"][1] - 1)}),
    ("doc outside the shard or level", set(), {"docs": lambda a: _changed(a, "docs", int(a["offs"][1]) - 1, a["bad_doc"])}),
    ("docs not ascending", set(), {"docs": _swapped}),
    ("tf = 0", set(), {"tfs": lambda a: _changed(a, "tfs", int(a["offs"][1]), 0)}),
    ("field = n_fields", {"fields"}, {"fields": lambda a: _changed(a, "fields", int(a["offs"][2]), 2)}),
    ("n_fields = 0", {"n_fields"}, {"n_fields": lambda a: 0}),
    ("n_fields = 1", {"n_fields"}, {"n_fields": lambda a: 1}),
    ("n_fields = 9", {"n_fields"}, {"n_fields": lambda a: 9}),
    ("n_positions = sum(tf) - 1", {"positions"}, {"positions": lambda a: a["positions_all"], "n_positions": lambda a: len(a["positions_all"]) - 1}),
    ("positions null, n_positions > 0", {"positions"}, {"positions": lambda a: None, "n_positions": lambda a: len(a["positions_all"])}),
    # (ss_bm25_append_sparse_positions takes the positions of a one-field tier as they come)
    ("positions not ascending inside a posting", set(e for e in ENTRY if "positions" in PARAMS[e]) - {"append_sparse_positions"},
     {"positions": _repeated, "n_positions": lambda a: len(a["positions_all"])}),
    ("level gap", {"level"}, {"level": lambda a: 3}),
    ("level neither next nor last", {"level"}, {"level": lambda a: 0}),
    ("level behind a partial one", {"level"}, {"level": lambda a: 2}),
    # (ss_bm25_append_level_fields lets a re-committed level shrink the vocabulary)
    ("shrinking vocabulary", {"append_level", "append_level_positions", "append_sparse_level"}, {"n_terms": lambda a: a["n_terms"] - 1}),
    ("positions on some levels only", {"append_level", "append_level_positions"}, {"shard": lambda a: a["other"]}),
    ("image uploaded whole", set(LEVELS) | {"append_sparse_level"}, {"shard": lambda a: "whole"}),
    ("no image", set(ENTRY) - set(UPLOADS), {"shard": lambda a: "empty"}),
    ("image of the other kind", set(SPARSE), {"shard": lambda a: a["other"]}),
    ("tier of levels", {"append_sparse", "append_sparse_positions"}, {"shard": lambda a: "tiered"}),
    ("grown vocabulary beside a tier", {"append_level", "append_level_positions"},
     {"shard": lambda a: "tiered", "n_terms": lambda a: a["n_terms"] + 1, "offs": _one_more_term}),
    ("commit beside a tier", {"append_level_fields"}, {"shard": lambda a: "tieredf"}),
]


def _applies(row, entry):
    to = row[1]
    return entry in to if to and to <= set(ENTRY) else to <= PARAMS[entry]


# CODES[entry][i][j], i <= j, over the rows that go to the entry: the code of rows i and j together (i == j: row i alone) in LETTER's
# letters (uploads: lower case where the old image is gone); '.': the two rows override the same argument.  The codes of 5f760f3.
CODES = {
    "upload": [
        "IIIIIIIIII",  # null shard
        " IIIII.III",  # null offs
        "  IIIII..I",  # null docs
        "   IIIIII.",  # null tfs
        "    IIIIII",  # n_terms = 0
        "     IIIII",  # n_docs = 0
        "      iiii",  # decreasing offs
        "       i.i",  # doc outside the shard or level
        "        ii",  # docs not ascending
        "         i",  # tf = 0
    ],
    "upload_positions": [
        "IIIIIIIIIIIII",  # null shard
        " IIIII.IIIIII",  # null offs
        "  IIIII..IIII",  # null docs
        "   IIIIII.III",  # null tfs
        "    IIIIIIIII",  # n_terms = 0
        "     IIIIIIII",  # n_docs = 0
        "      iiiIIIi",  # decreasing offs
        "       i.IIIi",  # doc outside the shard or level
        "        iIIIi",  # docs not ascending
        "         IiII",  # tf = 0
        "          I..",  # n_positions = sum(tf) - 1
        "           I.",  # positions null, n_positions > 0
        "            i",  # positions not ascending inside a posting
    ],
    "upload_fields": [
        "IIIIIIIIIIIIIII",  # null shard
        " IIIIII.IIIIIII",  # null offs
        "  IIIIII..IIIII",  # null docs
        "   IIIIIII.IIII",  # null tfs
        "    IIIIIII.III",  # null fields
        "     IIIIIIIIII",  # n_terms = 0
        "      IIIIIIIII",  # n_docs = 0
        "       IIIIIIII",  # decreasing offs
        "        i.iIIII",  # doc outside the shard or level
        "         IIIIII",  # docs not ascending
        "          iIIII",  # tf = 0
        "           IIII",  # field = n_fields
        "            I..",  # n_fields = 0
        "             I.",  # n_fields = 1
        "              I",  # n_fields = 9
    ],
    "upload_fields_positions": [
        "IIIIIIIIIIIIIIIIII",  # null shard
        " IIIIII.IIIIIIIIII",  # null offs
        "  IIIIII..IIIIIIII",  # null docs
        "   IIIIIII.IIIIIII",  # null tfs
        "    IIIIIII.IIIIII",  # null fields
        "     IIIIIIIIIIIII",  # n_terms = 0
        "      IIIIIIIIIIII",  # n_docs = 0
        "       IIIIIIIIIII",  # decreasing offs
        "        i.IIIIIIIi",  # doc outside the shard or level
        "         IIIIIIIII",  # docs not ascending
        "          IIIIIIII",  # tf = 0
        "           IIIIIII",  # field = n_fields
        "            I..III",  # n_fields = 0
        "             I.III",  # n_fields = 1
        "              IIII",  # n_fields = 9
        "               I..",  # n_positions = sum(tf) - 1
        "                I.",  # positions null, n_positions > 0
        "                 i",  # positions not ascending inside a posting
    ],
    "append_level": [
        "IIIIIIIIIIIIIII....",  # null shard
        " IIIIII.IIIIIIIIII.",  # null offs
        "  IIIIII..IIIIIIIII",  # null docs
        "   IIIIIII.IIIIIIII",  # null tfs
        "    IIIIIIIIII.III.",  # n_terms = 0
        "     I.IIIIIIIIIIII",  # n_level_docs = 0
        "      IIIIIIIIIIIII",  # n_level_docs = 65537
        "       IIIIIIIIISI.",  # decreasing offs
        "        I.IIIIIISIN",  # doc outside the shard or level
        "         IIIIIIISIN",  # docs not ascending
        "          IIIIIISIN",  # tf = 0
        "           I..IISIN",  # level gap
        "            I.IISIN",  # level neither next nor last
        "             IIISIN",  # level behind a partial one
        "              IISI.",  # shrinking vocabulary
        "               I...",  # positions on some levels only
        "                S..",  # image uploaded whole
        "                 I.",  # no image
        "                  N",  # grown vocabulary beside a tier
    ],
    "append_level_positions": [
        "IIIIIIIIIIIIIIIIII....",  # null shard
        " IIIIII.IIIIIIIIIIIII.",  # null offs
        "  IIIIII..IIIIIIIIIIII",  # null docs
        "   IIIIIII.IIIIIIIIIII",  # null tfs
        "    IIIIIIIIIIIII.III.",  # n_terms = 0
        "     I.IIIIIIIIIIIIIII",  # n_level_docs = 0
        "      IIIIIIIIIIIIIIII",  # n_level_docs = 65537
        "       IIIIIIIIIIIISI.",  # decreasing offs
        "        I.IIIIIIIIISIN",  # doc outside the shard or level
        "         IIIIIIIIIISIN",  # docs not ascending
        "          IIIIIIIIISIN",  # tf = 0
        "           I..IIIIISIN",  # n_positions = sum(tf) - 1
        "            I.IIIIIIII",  # positions null, n_positions > 0
        "             IIIIIISIN",  # positions not ascending inside a posting
        "              I..IISIN",  # level gap
        "               I.IISIN",  # level neither next nor last
        "                IIISIN",  # level behind a partial one
        "                 IISI.",  # shrinking vocabulary
        "                  I...",  # positions on some levels only
        "                   S..",  # image uploaded whole
        "                    I.",  # no image
        "                     N",  # grown vocabulary beside a tier
    ],
    "append_level_fields": [
        "IIIIIIIIIIIIIIIIIII...",  # null shard
        " IIIIIII.IIIIIIIIIIIII",  # null offs
        "  IIIIIII..IIIIIIIIIII",  # null docs
        "   IIIIIIII.IIIIIIIIII",  # null tfs
        "    IIIIIIII.IIIIIIIII",  # null fields
        "     IIIIIIIIIIIIIIIII",  # n_terms = 0
        "      I.IIIIIIIIIIIIII",  # n_level_docs = 0
        "       IIIIIIIIIIIIIII",  # n_level_docs = 65537
        "        IIIIIIIIIIISIN",  # decreasing offs
        "         I.IIIIIIIISIN",  # doc outside the shard or level
        "          IIIIIIIIISIN",  # docs not ascending
        "           IIIIIIIISIN",  # tf = 0
        "            IIIIIIISIN",  # field = n_fields
        "             I..IIIIII",  # n_fields = 0
        "              I.IIIIII",  # n_fields = 1
        "               IIIIIII",  # n_fields = 9
        "                I..SIN",  # level gap
        "                 I.SIN",  # level neither next nor last
        "                  ISIN",  # level behind a partial one
        "                   S..",  # image uploaded whole
        "                    I.",  # no image
        "                     N",  # commit beside a tier
    ],
    "append_sparse_level": [
        "IIIIIIIIIIIIIIII..",  # null shard
        " IIII.IIIIIIIIIIII",  # null offs
        "  IIII..IIIIIIIIII",  # null docs
        "   IIIII.IIIIIIIII",  # null tfs
        "    IIIIIIIIIII.II",  # n_terms = 0
        "     IIIIIIIIIIISS",  # decreasing offs
        "      I.IIIIIIIISS",  # doc outside the shard or level
        "       IIIIIIIIISS",  # docs not ascending
        "        IIIIIIIISS",  # tf = 0
        "         I..IIIISS",  # n_positions = sum(tf) - 1
        "          I.IIIISS",  # positions null, n_positions > 0
        "           IIIIISS",  # positions not ascending inside a posting
        "            I..ISS",  # level gap
        "             I.ISS",  # level neither next nor last
        "              IISS",  # level behind a partial one
        "               ISS",  # shrinking vocabulary
        "                S.",  # image uploaded whole
        "                 S",  # no image
    ],
    "append_sparse": [
        "IIIIIIII...",  # null shard
        " III.IIIIII",  # null offs
        "  III..IIII",  # null docs
        "   IIII.III",  # null tfs
        "    IIIISNI",  # decreasing offs
        "     I.ISNI",  # doc outside the shard or level
        "      IISNI",  # docs not ascending
        "       ISNI",  # tf = 0
        "        S..",  # no image
        "         N.",  # image of the other kind
        "          S",  # tier of levels
    ],
    "append_sparse_fields": [
        "IIIIIIIIII..",  # null shard
        " IIII.IIIIII",  # null offs
        "  IIII..IIII",  # null docs
        "   IIIII.III",  # null tfs
        "    IIIII.II",  # null fields
        "     IIIIISI",  # decreasing offs
        "      I.IISI",  # doc outside the shard or level
        "       IIISI",  # docs not ascending
        "        IISI",  # tf = 0
        "         ISI",  # field = n_fields
        "          S.",  # no image
        "           I",  # image of the other kind
    ],
    "append_sparse_positions": [
        "IIIIIIIIII...",  # null shard
        " III.IIIIIIII",  # null offs
        "  III..IIIIII",  # null docs
        "   IIII.IIIII",  # null tfs
        "    IIIIIISNI",  # decreasing offs
        "     I.IIISNI",  # doc outside the shard or level
        "      IIIISNI",  # docs not ascending
        "       IIISNI",  # tf = 0
        "        I.SNS",  # n_positions = sum(tf) - 1
        "         IIII",  # positions null, n_positions > 0
        "          S..",  # no image
        "           N.",  # image of the other kind
        "            S",  # tier of levels
    ],
    "append_sparse_fields_positions": [
        "IIIIIIIIIIIII..",  # null shard
        " IIII.IIIIIIIII",  # null offs
        "  IIII..IIIIIII",  # null docs
        "   IIIII.IIIIII",  # null tfs
        "    IIIII.IIIII",  # null fields
        "     IIIIIIIISI",  # decreasing offs
        "      I.IIIIISI",  # doc outside the shard or level
        "       IIIIIISI",  # docs not ascending
        "        IIIIISI",  # tf = 0
        "         IIIISI",  # field = n_fields
        "          I..SI",  # n_positions = sum(tf) - 1
        "           I.II",  # positions null, n_positions > 0
        "            ISI",  # positions not ascending inside a posting
        "             S.",  # no image
        "              I",  # image of the other kind
    ],
}


@pytest.fixture(scope="module")
def S():
    import seekstorm_amd
    return seekstorm_amd


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


def N():
    from seekstorm_amd import _native
    return _native


def _positions(tfs):
    """every posting's positions 0 .. tf - 1"""
    t = tfs.astype(np.int64)
    return (np.arange(int(t.sum())) - np.repeat(np.cumsum(t) - t, t)).astype(np.uint16)


def _field_level(c, lo, hi):
    dl, offs, docs, fields, tfs = c
    m = (docs >= lo) & (docs < hi)
    o = np.zeros(len(offs), np.uint64)
    o[1:] = np.cumsum([int(m[int(offs[t]):int(offs[t + 1])].sum()) for t in range(len(offs) - 1)])
    return np.ascontiguousarray(dl[:, lo:hi]), o, docs[m], fields[m], tfs[m]


class World:
    pass


@pytest.fixture(scope="module")
def W(S, O):
    W = World()
    dl = O.lex_doclen(N_DOCS)
    offs, docs, tfs = O.lex_corpus(N_DOCS, VOC)
    tfs[int(offs[3]):int(offs[4])] = np.maximum(tfs[int(offs[3]):int(offs[4])], 2)  # (term 3: two positions or more in every posting)
    W.one = (dl, offs, docs, tfs)
    W.levels = _level_slices(N_DOCS, offs, docs, tfs)
    fc = _fields_corpus(O, N_DOCS, 2, DFS, 77)
    fc[4][int(fc[1][3]):int(fc[1][4])] = np.maximum(fc[4][int(fc[1][3]):int(fc[1][4])], 2)
    W.two = fc
    W.flevels = [_field_level(fc, 0, FULL), _field_level(fc, FULL, N_DOCS)]
    rng = np.random.default_rng(5)
    sizes = [40, 7, 300, 25]
    s_docs = np.concatenate([np.sort(rng.choice(np.arange(FULL, N_DOCS), n, replace=False)) for n in sizes]).astype(np.uint32)
    s_tfs = np.minimum(rng.geometric(0.5, len(s_docs)), 5).astype(np.uint16)
    s_tfs[-sizes[3]:] = np.maximum(s_tfs[-sizes[3]:], 2)
    W.rare = (np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64), s_docs, (s_docs & 1).astype(np.uint8), s_tfs)
    for o in (W.levels[1][2], W.flevels[1][1], W.rare[0]):
        assert o[1] - o[0] >= 4 and np.all(o[1:4] < o[2:5])  # (the rows change postings of the first four lists)
    W.shards = {}
    try:
        for name in ("empty", "scratch", "whole", "wholef", "main", "mainp", "mainf", "tiered", "tieredf"):
            sh = W.shards[name] = S.Shard(0)
            if name == "whole":
                sh.upload_lexical(N_DOCS, dl, offs, docs, tfs)
            if name == "wholef":
                sh.upload_lexical_fields(N_DOCS, fc[0], BOOST, *fc[1:])
            if name in ("main", "mainp", "tiered"):
                for lv, (lo, hi, lo_, do_, to_) in enumerate(W.levels):
                    sh.append_level(lv, dl[lo:hi], lo_, do_, to_, positions=_positions(to_) if name == "mainp" else None)
            if name in ("mainf", "tieredf"):
                for lv, (ldl, lo_, ld, lf, lt) in enumerate(W.flevels):
                    sh.append_level_fields(lv, ldl, BOOST, lo_, ld, lf, lt)
            if name == "tiered":
                sh.append_sparse_level(1, W.rare[0], W.rare[1], W.rare[3])
            if name == "tieredf":
                assert sh.append_sparse_fields(*W.rare) == len(VOC)
        yield W
    finally:
        for sh in W.shards.values():
            sh.close()


def valid(W, entry):
    """the arguments of the entry's valid call, and what the rows need to know about them"""
    fields = "fields" in PARAMS[entry]
    if entry in UPLOADS:
        dl, offs, docs, f, tfs = W.two if fields else (*W.one[:3], None, W.one[3])
        a = {"shard": "scratch", "n_docs": N_DOCS, "bad_doc": N_DOCS}
    elif entry in LEVELS:
        dl, offs, docs, f, tfs = W.flevels[1] if fields else (W.one[0][FULL:], *W.levels[1][2:4], None, W.levels[1][4])
        a = {"shard": {"append_level": "main", "append_level_positions": "mainp", "append_level_fields": "mainf"}[entry], "level": 1,
             "n_level_docs": PART, "bad_doc": FULL - 1, "other": "mainp" if entry == "append_level" else "main"}
    else:
        dl, (offs, docs, f, tfs) = None, W.rare
        a = {"shard": "tiered" if entry == "append_sparse_level" else "wholef" if fields else "whole", "level": 1, "bad_doc": N_DOCS,
             "other": "whole" if fields else "wholef", "first": np.zeros(1, np.uint32)}
    pos = _positions(tfs)
    a.update(doclen=None if dl is None else np.ascontiguousarray(dl).reshape(-1), n_terms=len(offs) - 1, offs=offs, docs=docs, tfs=tfs, fields=f,
             n_fields=2, boost=BOOST, npos=None, positions_all=pos)
    with_pos = "positions" in PARAMS[entry] and entry != "append_sparse_level"  # (`tiered` has no positions: its valid call brings none)
    a.update(positions=pos if with_pos else None, n_positions=len(pos) if with_pos else 0)
    first = int(offs[0])
    a["swap_at"] = first + int(np.flatnonzero(docs[first:int(offs[1]) - 2] != docs[first + 1:int(offs[1]) - 1])[0])
    return a


TYPES = {"doclen": "u8p", "boost": "f32p", "offs": "u64p", "docs": "u32p", "fields": "u8p", "tfs": "u16p", "npos": "u16p", "positions": "u16p",
         "first": "u32p"}


def call(W, entry, rows=()):
    """the entry under its valid call's arguments with the rows' overrides written over them -> the code"""
    n, a = N(), valid(W, entry)
    over = {key: fn(a) for row in rows for key, fn in row[2].items()}
    a.update(over)
    name, params = ENTRY[entry]
    args = []
    for p in params.split():
        if p == "shard":
            args.append(None if a[p] is None else W.shards[a[p]]._h)
        elif p in TYPES:
            args.append(n.ptr(a[p], getattr(n, TYPES[p])))
        else:
            args.append(int(a[p]))
    return getattr(n.lib(), name)(*args)


def snapshot(S, sh):
    """what a refused call must leave as it was: the levels, ss_bm25_info, answers of unions and intersections under both strategies"""
    n = N()
    out = [sh.incremental_info()[0], sh.lexical_info()]
    for strategy in (n.BM25_AUTO, n.BM25_EXHAUSTIVE):
        sh.set_strategy(strategy)
        for qt in (S.QueryType.Union, S.QueryType.Intersection):
            out.append(sh.search_lexical_batch(sh.make_queries(QUERIES, qt), K))
    sh.set_strategy(n.BM25_AUTO)
    return out


def same(a, b):
    return a[:2] == b[:2] and all(np.array_equal(x, y) for p, q in zip(a[2:], b[2:]) for x, y in zip(p, q))


def has_image(W, shard):
    rc = N().lib().ss_bm25_info(W.shards[shard]._h, None, None, None, None)
    assert rc in (N().SS_OK, N().SS_ESTATE)
    return rc == N().SS_OK


def good_upload(W):
    dl, offs, docs, tfs = W.one
    W.shards["scratch"].upload_lexical(N_DOCS, dl, offs, docs, tfs, _positions(tfs))


def observe(S, W, entry):
    """the table of `entry` as the library answers it now, in CODES' form"""
    rows = [r for r in ROWS if _applies(r, entry)]
    table = []
    if entry in UPLOADS:
        good_upload(W)
        good = snapshot(S, W.shards["scratch"])
    for i, ri in enumerate(rows):
        line = " " * i
        for j in range(i, len(rows)):
            if i != j and set(ri[2]) & set(rows[j][2]):
                line += "."
                continue
            rc = call(W, entry, (ri,) if i == j else (ri, rows[j]))
            assert rc != 0, (entry, ri[0], rows[j][0], "accepted")
            if entry in UPLOADS and not has_image(W, "scratch"):
                line += LETTER[rc].lower()
                good_upload(W)
            else:
                line += LETTER[rc]
                if entry in UPLOADS and i == j:
                    assert same(snapshot(S, W.shards["scratch"]), good), (entry, ri[0])
        table.append(line)
    return [r[0] for r in rows], table


@pytest.mark.parametrize("entry", list(ENTRY))
def test_codes_of_rows_and_pairs(S, W, entry):
    names, got = observe(S, W, entry)
    print("\n    \"%s\": [\n%s\n    ]," % (entry, "\n".join('        "%s",  # %s' % (line, name) for line, name in zip(got, names))))
    want = CODES[entry]
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        for j in range(i, len(names)):
            assert g[j] == w[j], (entry, names[i], names[j], g[j], w[j])


@pytest.mark.parametrize("entry", LEVELS)
def test_a_refused_commit_changes_nothing(S, W, entry):
    """every row that goes to the entry, alone: refused before the swap, and the image of the shard the call went to -- two levels, the
    second one partial -- answers as before, bit for bit"""
    before = {name: snapshot(S, W.shards[name]) for name in ("main", "mainp", "mainf", "tiered", "tieredf", "whole")}
    for name, snap in before.items():
        assert snap[0] == (0 if name == "whole" else 2) and snap[1]["n_docs"] == N_DOCS and all(int(x[3].max()) > 0 for x in snap[2:]), name
    assert not same(before["main"], before["mainf"])
    for row in ROWS:
        if not _applies(row, entry):
            continue
        rc = call(W, entry, (row,))
        assert rc != 0, (entry, row[0])
        went_to = row[2]["shard"](valid(W, entry)) if "shard" in row[2] else valid(W, entry)["shard"]
        if went_to in before:
            assert same(snapshot(S, W.shards[went_to]), before[went_to]), (entry, row[0], went_to)
    for name, snap in before.items():
        assert same(snapshot(S, W.shards[name]), snap), (entry, name)
    assert not has_image(W, "empty")
