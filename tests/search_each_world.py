"""The small image tests/test_gpu_search_each.py and tests/test_gpu_faceted_callers.py share (imported, not collected): 143 397 docs --
two full levels, three sub-blocks and 37 docs, so the image crosses a level edge and a sub-block edge and is no multiple of 32 or 64 --,
48 dense terms with df from 0.05 % to 40 % and positions (every tf is 1), a sparse tier of 300 rare terms, 1 % tombstones with doc 0 and
the last doc among them, facet records of 24 bytes (u32 @0, i16 @4, string16 @6 with 40 ids, f32 @8, point @16) and a rank table for
the string field.  With it: 71 queries (two chunks, 64 + 7), nine facet-filter sets with their statement in numpy, three query_facets
and a two-field sort."""
import numpy as np

N_DOCS = 2 * 65536 + 3 * 4096 + 37
N_DENSE, N_SPARSE, N_IDS = 48, 300, 40
REC = np.dtype({"names": ["u32", "i16", "s16", "f32", "loc"], "formats": ["<u4", "<i2", "<u2", "<f4", "<u8"], "offsets": [0, 4, 6, 8, 16], "itemsize": 24})
OFF = {n: REC.fields[n][1] for n in REC.names}
BASE, UNIT = (38.8951, 30.25), "km"
OR, AND, PHRASE = "or", "and", "phrase"
STRINGS = ["s%02d" % ((i * 7) % 37) for i in range(N_IDS)]  # (ids 37 apart share a string: equal ranks)
EXTERN_IDS = list(range(0, 60, 2))  # 30 ids: more than the 8 a filter holds inline


class World:
    pass


def build(S, O, positions=True, oracle=True):
    rng = np.random.default_rng(20240607)
    W = World()
    W.n_docs = N_DOCS
    W.dl = O.lex_doclen(N_DOCS)
    dfs = np.geomspace(0.0005, 0.40, N_DENSE)[::-1]  # term 0 the most frequent
    lists = [np.sort(rng.choice(N_DOCS, max(int(df * N_DOCS), 1), replace=False)).astype(np.uint32) for df in dfs]
    lists[5] = np.union1d(lists[5], [0, 63, 64, 4095, 4096, 65535, 65536, N_DOCS - 1]).astype(np.uint32)  # the edges hold a match
    W.offs = np.concatenate([[0], np.cumsum([len(d) for d in lists])]).astype(np.uint64)
    W.docs = np.concatenate(lists)
    W.tfs = np.ones(len(W.docs), np.uint16)
    # one position per posting: term t at 40 + t, but term 0 at 5 and term 1 at 6 in the docs divisible by 3 (9 elsewhere) -- the phrase
    # [0, 1] stands in those docs of both lists, and its intersection holds docs without it
    pos = [np.full(len(d), 40 + t, np.uint16) for t, d in enumerate(lists)]
    pos[0][:] = 5
    pos[1] = np.where(lists[1] % 3 == 0, 6, 9).astype(np.uint16)
    W.pos = np.concatenate(pos)
    sl = [np.sort(rng.choice(N_DOCS, int(rng.integers(3, 41)), replace=False)).astype(np.uint32) for _ in range(N_SPARSE)]
    s_offs = np.concatenate([[0], np.cumsum([len(d) for d in sl])]).astype(np.uint64)
    s_docs, s_tfs = np.concatenate(sl), np.ones(int(s_offs[-1]), np.uint16)
    v = np.zeros(N_DOCS, REC)
    v["u32"] = rng.integers(0, 1 << 32, N_DOCS, dtype=np.uint64)
    v["i16"] = rng.integers(-32768, 32768, N_DOCS)
    v["i16"][::97] = 32767
    v["i16"][1::97] = -32768
    v["s16"] = rng.integers(0, N_IDS, N_DOCS)
    f = rng.normal(0.0, 50.0, N_DOCS)
    v["f32"] = np.where(rng.integers(0, 4, N_DOCS) == 0, np.array([0.0, -0.0, 1.0, -1.0])[rng.integers(0, 4, N_DOCS)], f).astype(np.float32)
    v["loc"] = O.morton_encode(rng.random(N_DOCS) * 50.0 + 10.0, rng.random(N_DOCS) * 60.0 + 5.0)
    W.v, W.off = v, OFF
    W.gone = sorted(set(rng.choice(N_DOCS, N_DOCS // 100, replace=False).tolist()) | {0, N_DOCS - 1})
    W.sh = S.Shard(0)
    W.sh.upload_lexical(N_DOCS, W.dl, W.offs, W.docs, W.tfs, W.pos if positions else None)
    assert W.sh.append_sparse(s_offs, s_docs, s_tfs, positions=np.full(len(s_docs), 7, np.uint16) if positions else None) == N_DENSE
    W.sh.upload_facets(np.ascontiguousarray(v.view(np.uint8).reshape(N_DOCS, REC.itemsize)))
    W.sh.set_string_facet_ranks(OFF["s16"], "string16", STRINGS)
    W.sh.set_deleted(W.gone)
    if oracle:
        W.osh = O.Shard(N_DOCS, W.dl, np.concatenate([W.offs, W.offs[-1] + s_offs[1:]]), np.concatenate([W.docs, s_docs]), np.concatenate([W.tfs, s_tfs]))
        W.osh.set_positions(np.concatenate([W.pos, np.full(len(s_docs), 7, np.uint16)]))
        W.dist = O.geo_distances(v["loc"], BASE, UNIT)
    return W


def queries():
    """71 (op, terms, NOT terms): 1-4-term ANDs and ORs, one 6-term OR, one phrase, two naming a sparse term, one with a NOT term"""
    rng = np.random.default_rng(5)
    qs = [(OR, [0, 3, 7, 12, 20, 33], []), (PHRASE, [0, 1], []), (OR, [2, N_DENSE + 4], []), (AND, [N_DENSE + 9], []), (OR, [1, 6], [2]), (OR, [5], [])]
    while len(qs) < 71:
        n = int(rng.integers(1, 5))
        if rng.random() < 0.5:  # intersections of frequent terms, so that most of them match something under a filter as well
            qs.append((AND, [int(t) for t in rng.permutation(8)[:n]], []))
        else:
            qs.append((OR, [int(t) for t in rng.permutation(N_DENSE)[:n]], []))
    return qs


def make(S, W, qs):
    ty = {OR: S.QueryType.Union, AND: S.QueryType.Intersection, PHRASE: S.QueryType.Phrase}
    return W.sh.make_queries([t for _, t, _ in qs], [ty[op] for op, _, _ in qs], [n for _, _, n in qs])


def filter_sets(O, W):
    """the nine sets, dealt round-robin (query i runs under set i % 9): (name, the mirror's filter list, the docs that pass)"""
    v = W.v
    m0, m1 = O.geo_morton_range(BASE, 1500.0, UNIT)
    ids = [1, 3, 5, 7, 11, 13, 17, 19]
    two = [(OFF["u32"], "u32", 1 << 28, 7 << 29), (OFF["f32"], "f32", -10.0, 80.0)]
    two_keep = (v["u32"] >= (1 << 28)) & (v["u32"] < (7 << 29)) & (v["f32"] >= np.float32(-10.0)) & (v["f32"] < np.float32(80.0))
    every = np.ones(W.n_docs, bool)
    return [
        ("none", [], every),
        ("nothing", [(OFF["u32"], "u32", 5, 5)], ~every),
        ("everything", [(OFF["u32"], "u32", 0, 1 << 32)], every),
        ("i16 extremes", [(OFF["i16"], "i16", -32768, 32767)], v["i16"] < 32767),
        ("8 ids", [(OFF["s16"], "string16", ids)], np.isin(v["s16"], ids)),
        ("point", [(OFF["loc"], "point", BASE, 200.0, 1500.0, UNIT)],
         (v["loc"] >= np.uint64(m0)) & (v["loc"] < np.uint64(m1)) & (W.dist >= 200.0) & (W.dist < 1500.0)),
        ("two", two, two_keep),
        ("two again", list(two), two_keep),
        ("30 extern ids", [(OFF["s16"], "string16", EXTERN_IDS)], np.isin(v["s16"], EXTERN_IDS)),
    ]


def _ranges(bounds):
    return [("r%d" % i, b) for i, b in enumerate(bounds)]


def facets():
    return [
        {"field": "u32", "offset": OFF["u32"], "type": "u32", "ranges": _ranges([5, 1 << 30, 1 << 31, (1 << 32) - 1000]), "range_type": "within"},
        {"field": "s16", "offset": OFF["s16"], "type": "string16", "values": ["a%d" % i for i in range(N_IDS)], "prefix": "", "length": 10},
        {"field": "loc", "offset": OFF["loc"], "type": "point", "ranges": _ranges([0.0, 500.0, 1000.0, 2000.0, 3000.0]), "range_type": "within",
         "base": BASE, "unit": UNIT},
    ]


SORTS = [(OFF["s16"], "string16", False), (OFF["f32"], "f32", True)]
