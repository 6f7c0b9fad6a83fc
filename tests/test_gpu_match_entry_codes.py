"""Return codes of the entries that walk a match set, for bad and borderline inputs alone and in pairs (csrc/ss_api.hip; -m gpu).

ss_bm25_facet_count, ss_bm25_facet_kth, ss_bm25_search_sorted, ss_bm25_search_facets and ss_docs_search check their arguments, the
shard's state and the batch's queries in an order that is part of their behaviour: which refusal wins when two apply.  One table of
rows (ROWS), every row an override of one valid call; every row alone and every pair of rows goes to every entry that takes all of
the overridden arguments, and the code is compared with a literal.  The literals (CODES) are the codes commit 1d0c343 returns:
read off the order of its checks first, then confirmed by running this test against a build of that commit.

One world: test_gpu_tier_facets.py's corpus (5 dense + 9 sparse lists) and facet record over 8 003 docs, with tombstones, on four
shards -- `main` (positions in both tiers), `bare` (no positions), `rationed` (a probe budget of three rows and the all-zero row, no
pool: the dense lists 0 and 1 have no row; a budget of 0 bytes itself selects the default, under which every list has one) and
`nofacets` (no facet records).  Every row is an argument or state refusal that returns before any launch, or a small valid call.

After a refusal the shard the call went to answers the entry's valid call as it did before (on `nofacets`, where no entry has one,
the plain search): the answers of the valid calls are checked once against numpy / oracle/naive.py and compared bit for bit afterwards."""
import ctypes as C

import numpy as np
import pytest

from oracle import naive
from test_gpu_facet_edges import REC, World, _reference_order, check_sorted, value_of
from test_gpu_tier_facets import ND, NS, _columns, _tiered_corpus

pytestmark = pytest.mark.gpu

N_DOCS = 8_003
K = 10
I32, STRING16, POINT = 6, 10, 12
SORT = [("i32", True)]
ROWS = ["term beyond the vocabulary", "duplicate term", "phrase, image without positions", "list without a probe row", "offset at record_size - width + 1",
        "facet type 13", "n_buckets = 0", "missing bounds", "Point facet without a base", "string sort field", "no facet records", "nq = 0", "k = 0"]
# what an entry takes of a row's overrides; a row or pair that overrides anything else is not that entry's ('.')
TAKES = {"count": {"shard", "query", "offset", "ftype", "base", "n_buckets", "bounds"},
         "kth": {"shard", "query", "offset", "ftype", "base", "sort_type", "k"},
         "sorted": {"shard", "query", "offset", "ftype", "sort_type", "nq", "k"},
         "facets": {"shard", "query", "offset", "ftype", "base", "n_buckets", "bounds", "nq", "k"},
         "docs": {"shard", "offset", "ftype", "base", "n_buckets", "bounds", "sort_type", "k"}}
LETTER = {0: "K", -1: "I", -2: "M", -3: "D", -4: "N", -5: "S"}  # OK, EINVAL, ENOMEM, EDEVICE, ENOTSUP, ESTATE
# CODES[entry][i][j], i <= j: the code of rows i and j together (i == j: row i alone) in LETTER's letters; '.': not this entry's, or
# the two rows override the same argument.  The codes of 1d0c343.
CODES = {
    "count": [
        "I...IIIII.I..",
        " I..IIIII.I..",
        "  N.NIIII....",
        "   NNIIII....",
        "    SIIII.S..",
        "     III..I..",
        "      III.I..",
        "       II.I..",
        "        I.I..",
        "         ....",
        "          S..",
        "           ..",
        "            .",
    ],
    "kth": [
        "I...II..INI.I",
        " I..II..INI.I",
        "  N.NI..IN..I",
        "   NNI..IN..I",
        "    SI..INS.I",
        "     I....I.I",
        "      .......",
        "       ......",
        "        I.I.I",
        "         NN.I",
        "          S.I",
        "           ..",
        "            I",
    ],
    "sorted": [
        "I...SI...NSII",
        " I..SI...NSII",
        "  N.SI...N.II",
        "   NSI...N.II",
        "    SI...NSII",
        "     I....III",
        "      .......",
        "       ......",
        "        .....",
        "         NNII",
        "          SII",
        "           II",
        "            I",
    ],
    "facets": [
        "I...SIIII.SKI",
        " I..SIIII.SKI",
        "  N.SIIII..KI",
        "   NSIIII..KI",
        "    SIIII.SKI",
        "     III..III",
        "      III.III",
        "       II.III",
        "        I.III",
        "         ....",
        "          SKI",
        "           KI",
        "            I",
    ],
    "docs": [
        ".............",
        " ............",
        "  ...........",
        "   ..........",
        "    IIIIIIS.I",
        "     III.II.I",
        "      IIIII.I",
        "       IIII.I",
        "        III.I",
        "         II.I",
        "          S.I",
        "           ..",
        "            I",
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


def _positions(tfs):
    """every posting's positions 0 .. tf - 1"""
    t = tfs.astype(np.int64)
    return (np.arange(int(t.sum())) - np.repeat(np.cumsum(t) - t, t)).astype(np.uint16)


@pytest.fixture(scope="module")
def W(S, O):
    W = World()
    W.raw = _columns(W, N_DOCS, 2027)
    dl, d_offs, d_docs, d_tfs, s_offs, s_docs, s_tfs, hot = _tiered_corpus(O, N_DOCS, 21)
    W.osh = O.Shard(N_DOCS, dl, np.concatenate([d_offs, d_offs[-1] + s_offs[1:]]), np.concatenate([d_docs, s_docs]), np.concatenate([d_tfs, s_tfs]))
    W.gone = sorted(set(hot[::5].tolist()) | set(range(13, N_DOCS, 97)))
    W.osh.set_deleted(W.gone)
    W.shards = {}
    try:
        for name in ("main", "bare", "rationed", "nofacets"):
            sh = W.shards[name] = S.Shard(0)
            if name == "rationed":
                sh.set_probe_budget(4 * ((N_DOCS + 4095) // 4096) * 64 * 12)
            sh.upload_lexical(N_DOCS, dl, d_offs, d_docs, d_tfs, _positions(d_tfs) if name == "main" else None)
            assert sh.append_sparse(s_offs, s_docs, s_tfs, positions=_positions(s_tfs) if name == "main" else None) == ND
            if name != "nofacets":
                sh.upload_facets(W.raw)
            sh.set_deleted(W.gone)
        assert W.shards["rationed"].terms_probed([0, 1, 2, 3, 4]).tolist() == [0, 0, 1, 1, 1]
        W.bounds = np.array([int(x) & 0xFFFFFFFFFFFFFFFF for x in W.vals["i32"][1::3]], np.uint64)
        main = W.shards["main"]
        W.q_ok = main.make_queries([[4, 9]], S.QueryType.Intersection)
        W.q_beyond = W.q_ok.copy()
        W.q_beyond["term"][0, 1] = ND + NS
        W.q_dup = W.q_ok.copy()
        W.q_dup["term"][0, 1] = 4
        W.q_phrase = main.make_queries([[3, 4]], S.QueryType.Phrase)
        W.q_rowless = main.make_queries([[1, 8]], S.QueryType.Union)
        edge = REC.itemsize - 4 + 1  # an i32 there would end one byte behind the record
        W.rows = [{"query": W.q_beyond}, {"query": W.q_dup}, {"shard": "bare", "query": W.q_phrase}, {"shard": "rationed", "query": W.q_rowless},
                  {"offset": edge}, {"ftype": 13}, {"n_buckets": 0}, {"bounds": None}, {"ftype": POINT, "base": None}, {"sort_type": STRING16},
                  {"shard": "nofacets"}, {"nq": 0}, {"k": 0}]
        assert len(W.rows) == len(ROWS)
        yield W
    finally:
        for sh in W.shards.values():
            sh.close()


def _args(W, over):
    a = {"shard": "main", "query": W.q_ok, "offset": W.off["i32"], "ftype": I32, "n_buckets": len(W.bounds), "bounds": W.bounds, "nq": 1, "k": K}
    a.update(over)
    return a


def _sorts(a):
    arr = (N().ResultSortC * 1)()
    arr[0].facet_offset, arr[0].facet_type, arr[0].descending = a["offset"], a.get("sort_type", a["ftype"]), 1
    return arr


def N():
    from seekstorm_amd import _native
    return _native


def call(W, entry, over):
    """the entry under the valid call's arguments with `over` written over them -> (code, the raw outputs)"""
    n, a = N(), _args(W, over)
    L, h, q = n.lib(), W.shards[a["shard"]]._h, a["query"]
    qp = q.ctypes.data_as(C.c_void_p)
    point = a["ftype"] == POINT  # (always without a base here: the Point entries, or a null bases array)
    nb, bounds = a["n_buckets"], n.ptr(a["bounds"], n.u64p)
    doc, score = np.full(K, n.SS_NO_DOC, np.uint32), np.zeros(K, np.float32)
    cnt, tot = np.zeros(1, np.uint32), np.zeros(1, np.uint64)
    counts = np.zeros(len(W.bounds) + 1, np.uint64)
    off1, ty1, nb1 = np.array([a["offset"]], np.uint32), np.array([a["ftype"]], np.uint32), np.array([nb], np.uint32)
    if entry == "count":
        if point:
            rc = L.ss_bm25_facet_count_point(h, qp, 0, None, a["offset"], None, nb, bounds, n.ptr(counts, n.u64p), n.ptr(tot, n.u64p))
        else:
            rc = L.ss_bm25_facet_count(h, qp, 0, None, a["offset"], a["ftype"], nb, bounds, n.ptr(counts, n.u64p), n.ptr(tot, n.u64p))
        return rc, (counts, tot)
    if entry == "kth":
        v = np.zeros(3, np.uint64)
        p = [C.cast(v.ctypes.data + 8 * i, n.u64p) for i in range(3)]
        if point:
            rc = L.ss_bm25_facet_kth_point(h, qp, 0, None, a["offset"], None, 1, a["k"], p[0], p[1], p[2], n.ptr(tot, n.u64p))
        else:
            rc = L.ss_bm25_facet_kth(h, qp, 0, None, a["offset"], a.get("sort_type", a["ftype"]), 1, a["k"], p[0], p[1], p[2], n.ptr(tot, n.u64p))
        return rc, (v, tot)
    if entry == "sorted":
        rc = L.ss_bm25_search_sorted(h, a["nq"], qp, 1, C.cast(_sorts(a), C.c_void_p), a["k"], 0, None, n.ptr(doc, n.u32p), n.ptr(score, n.f32p),
                                     n.ptr(cnt, n.u32p), n.ptr(tot, n.u64p))
        return rc, (doc, score, cnt, tot)
    if entry == "facets":
        rc = L.ss_bm25_search_facets(h, a["nq"], qp, a["k"], n.RT_TOPKCOUNT, 0, None, 1, n.ptr(off1, n.u32p), n.ptr(ty1, n.u32p), n.ptr(nb1, n.u32p),
                                     bounds, None, n.ptr(doc, n.u32p), n.ptr(score, n.f32p), n.ptr(cnt, n.u32p), n.ptr(tot, n.u64p),
                                     n.ptr(counts, n.u64p))
        return rc, (doc, score, cnt, tot, counts)
    assert entry == "docs"
    srt = _sorts(dict(a, offset=W.off["i32"], ftype=I32))  # (the offset and type rows are the facet's; the sort field keeps its own)
    rc = L.ss_docs_search(h, 0, a["k"], n.RT_TOPKCOUNT, 0, 1, C.cast(srt, C.c_void_p), 0, None, 1, n.ptr(off1, n.u32p), n.ptr(ty1, n.u32p),
                          n.ptr(nb1, n.u32p), bounds, None, n.ptr(doc, n.u32p), n.ptr(cnt, n.u32p), n.ptr(tot, n.u64p), n.ptr(counts, n.u64p))
    return rc, (doc, cnt, tot, counts)


def _plain(W, shard):
    """the plain search of the valid query: what `nofacets` answers"""
    return W.shards[shard].search_lexical_batch(W.q_ok, K)


def _histogram(W, docs):
    b = [naive.facet_bucket(x, W.vals["i32"][1::3]) for x in W.vals["i32"]]
    want = np.zeros(len(W.bounds) + 1, np.int64)
    np.add.at(want, [len(W.bounds) if x is None else x for x in np.array(b, object)[W.idx["i32"][docs]]], 1)
    return want


@pytest.fixture(scope="module")
def good(S, O, W):
    """the valid call of every entry on every shard that has one, checked against the reference once"""
    md, ms, tot = W.osh.search_exhaustive([4, 9], O.OP_AND, N_DOCS)
    md = md.astype(np.int64)
    assert tot == len(md) > 3 * K
    live = np.setdiff1d(np.arange(N_DOCS), W.gone)
    vals = value_of(W, "i32", md)
    out = {}
    for shard in ("main", "bare", "rationed"):
        rc, (counts, t) = call(W, "count", {"shard": shard})
        assert rc == 0 and int(t[0]) == tot and np.array_equal(counts.astype(np.int64), _histogram(W, md)), shard
        out["count", shard] = (counts, t)
        rc, (v, t) = call(W, "kth", {"shard": shard})
        kv, kb, ke = naive.kth(vals, K, True)
        assert rc == 0 and int(t[0]) == tot and (int(v[1]), int(v[2])) == (kb, ke) and naive.facet_value(int(v[0]), "i32") == kv, shard
        out["kth", shard] = (v, t)
        rc, (doc, score, cnt, t) = call(W, "sorted", {"shard": shard})
        assert rc == 0
        check_sorted(W, doc[:cnt[0]], score[:cnt[0]], int(t[0]), _reference_order(W, md, ms, SORT), SORT, K, ("sorted", shard))
        out["sorted", shard] = (doc, score, cnt, t)
        rc, (doc, score, cnt, t, counts) = call(W, "facets", {"shard": shard})
        pd, ps, pc, pt = _plain(W, shard)
        assert rc == 0 and np.array_equal(doc, pd[0]) and np.array_equal(score, ps[0]) and cnt[0] == pc[0] and t[0] == pt[0] == tot, shard
        assert np.array_equal(counts.astype(np.int64), _histogram(W, md)), shard
        out["facets", shard] = (doc, score, cnt, t, counts)
        rc, (doc, cnt, t, counts) = call(W, "docs", {"shard": shard})
        key = np.array(value_of(W, "i32", live), np.int64)
        want = live[np.lexsort((-live, -key))][:K]  # i32 descending, then the larger doc id first
        assert rc == 0 and cnt[0] == K and int(t[0]) == len(live) and np.array_equal(doc, want), shard
        assert np.array_equal(counts.astype(np.int64), _histogram(W, live)), shard
        out["docs", shard] = (doc, cnt, t, counts)
    pd, ps, pc, pt = _plain(W, "nofacets")
    assert pt[0] == tot and np.array_equal(pd, _plain(W, "main")[0])
    out["plain"] = (pd, ps, pc, pt)
    assert call(W, "count", {"query": W.q_phrase})[0] == 0  # (with positions the phrase is answered: row 2 is about their absence)
    return out


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def observe(W, good, entry):
    """the table of `entry` as the library answers it now, in CODES' form -- and after every refusal the shard's valid call"""
    table = []
    for i in range(len(ROWS)):
        line = ""
        for j in range(len(ROWS)):
            over = dict(W.rows[i], **W.rows[j])
            one_type = entry in ("kth", "sorted") and {"ftype", "sort_type"} <= set(over)  # (their sort field IS the facet)
            if j < i or (i != j and set(W.rows[i]) & set(W.rows[j])) or not set(over) <= TAKES[entry] or one_type:
                line += "." if j >= i else " "
                continue
            rc = call(W, entry, over)[0]
            line += LETTER[rc]
            if rc != 0:
                shard = over.get("shard", "main")
                if shard == "nofacets":
                    assert _same(_plain(W, shard), good["plain"]), (entry, ROWS[i], ROWS[j])
                else:
                    rc2, got = call(W, entry, {"shard": shard})
                    assert rc2 == 0 and _same(got, good[entry, shard]), (entry, ROWS[i], ROWS[j], rc2)
        table.append(line)
    return table


@pytest.mark.parametrize("entry", list(TAKES))
def test_codes_of_rows_and_pairs(W, good, entry):
    got = observe(W, good, entry)
    print("\n".join('        "%s",' % line for line in got))  # (the table as it would be written into CODES)
    for i, (g, w) in enumerate(zip(got, CODES[entry])):
        for j in range(i, len(ROWS)):
            assert g[j] == w[j], (entry, ROWS[i], ROWS[j], g[j], w[j])
    assert len(got) == len(CODES[entry])


def test_search_facets_without_an_image_is_a_state_refusal_even_for_no_queries(S, W):
    """ss_bm25_search_facets: a shard without a lexical image is SS_ESTATE before nq == 0 is SS_OK (with an image: CODES, row "nq = 0")"""
    W.shards["empty"] = S.Shard(0)  # (closed with the others)
    for nq in (0, 1):
        assert call(W, "facets", {"shard": "empty", "nq": nq})[0] == N().SS_ESTATE
