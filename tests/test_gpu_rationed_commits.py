"""A RATIONED probe index (ss_bm25_set_probe_budget: rows for the longest lists, a quarter of them a pool filled on demand) on an image that
GROWS BY COMMITS.  The budget is in bytes and a row costs n_sub * 64 * 12 of them, so under one budget the row count falls as commits add
sub-blocks: one shard walks from unrationed, to rationed with a pool, to a smaller pool, to rationed without a pool -- and, under a budget
below two rows, has no probe index at all.  The new image's rows are built into blocks recycled from the old one, and the pool's host and
device tables are swapped with the image.

After every step the rationed, incrementally committed shard (`inc`) must answer exactly (np.array_equal, every output array) like
  `full` -- ONE upload of the same prefix with no budget (the header: both strategies return identical results), and like
  `one`  -- ONE upload of the prefix under the same budget, whose terms_probed must equal inc's right after the build: both builders
            deal the rows alike, and the rows they deal are the ones the header's rule gives (computed here from the dfs);
the CPU oracle anchors a few queries per world at the last step (totals exact, scores rtol 1e-4).

World A: one indexed field (ss_bm25_append_level_positions -> raw_fill_kernel).  World B: three indexed fields with merged lists
(ss_bm25_commit_level_fields -> mf_fill_kernel).  World C: both again with their rarest lists as a sparse tier
(ss_bm25_append_sparse_level / ss_bm25_commit_sparse_level_fields).  The generator's builder (ss_bm25_synth -> lex_gen_kernel) has its own
rationed case at the end.  A level is 65 536 docs and a sub-block 4096: two full levels, a partial third of 12 000 docs, the third
re-committed at 30 000 -- n_sub 16, 32, 35, 40."""
import numpy as np
import pytest

from test_gpu_commit_fields import Corpus, _edit

pytestmark = pytest.mark.gpu

LVL = 65536
PARTIAL = 12_000
N_DOCS = 2 * LVL + 30_000
# (level, first doc, end doc)
STEPS = [(0, 0, LVL), (1, LVL, 2 * LVL), (2, 2 * LVL, 2 * LVL + PARTIAL), (2, 2 * LVL, N_DOCS)]
N_SUB = [(hi + 4095) // 4096 for _, _, hi in STEPS]
ROW_BYTES = 64 * 12                 # per sub-block: 64 groups of 64 docs, a bit record (8 bytes) and a rank (4) each
BUDGET = 41 * 32 * ROW_BYTES        # 40 rows + the zero row at 32 sub-blocks
BUDGET_TIER_B = 33 * 32 * ROW_BYTES  # (36 virtual lists beside the tier: 32 rows at 32 sub-blocks keep it rationed with a pool)
NO_INDEX = 2 * 16 * ROW_BYTES - 1   # below two rows' bytes at the first step already: max_rows == 0 at every step
EDGE_DOCS = [0, 63, 64, 4095, 4096, LVL - 1, LVL] + [hi - 1 for _, _, hi in STEPS]  # edges of a 64-doc group, a sub-block, a level, a prefix
LONE_SB, HOLE_SB = 5, 21            # a sub-block the edge lists hold ONE posting in; one the rowed edge list holds none in
BAD = 0xFFFFFFFF
BOOST = [2.0, 1.0, 0.5]

# ---- world A: 48 lists, dfs falling geometrically from 8 % to 0.05 % of the docs
A_TERMS, A_EMPTY, A_DENSE_TIERED = 48, 39, 40
A_ABSENT_L1, A_L2_ONLY = 26, 10     # no posting in level 1; (almost) only in level 2: their rank by df moves from step to step
A_EDGE = (3, 34, 44)                # lists with postings on EDGE_DOCS: 3 always owns a row, 34 and 44 have none when rationed
A_BIG = [0, 1, 2, 3, 4, 5]          # the longest lists: a fixed row whenever there is an index
A_PLANT = [([1, 2], 300), ([2, 40], 60), ([45, 46], 60), ([36, 37, 45], 60), ([38, 40, 41, 42, 43, 44, 47], 60)]
A_PHRASES = [[1, 2], [2, 40], [45, 46], [36, 37, 45], [38, 40, 41, 42, 43, 44, 47], [46, 45], [2, 1, 2]]
A_SHORT_PHRASES = [[45, 46], [36, 37, 45]]  # over short lists only: no row when rationed

# ---- world B: 12 terms x (3 fields + merged) = 48 virtual lists
B_TERMS, B_EMPTY, B_DENSE_TIERED = 12, 8, 9
B_DFS = [14_000, 11_000, 8_500, 6_500, 5_000, 3_800, 2_900, 2_200, 0, 1_600, 1_100, 500]
B_ABSENT_L1 = 5
B_EDGE = (0, 7, 11)                # term 0 owns every row, 7 loses field rows when rationed, 11 all four
B_PLANT = [([0, 1], 0, 300), ([0, 1], 2, 200), ([7, 6], 1, 150), ([7, 6], 0, 150), ([9, 10], 1, 150), ([9, 10], 2, 150), ([6, 9, 10], 0, 120),
           ([6, 10], 1, 150), ([0, 7], 1, 120), ([11, 0], 2, 100), ([11, 7], 1, 100)]
B_CROSS = [(0, 1, 500), (9, 10, 100)]
B_PHRASES = [[0, 1], [1, 0], [7, 6], [9, 10], [6, 9, 10], [6, 10], [11, 0]]
B_PHRASES_IN = {(1,): [[7, 6], [9, 10], [6, 10], [0, 7]], (0, 2): [[0, 1], [7, 6], [9, 10], [6, 9, 10], [11, 0]]}  # planted in a listed field


@pytest.fixture(scope="module")
def S():
    import seekstorm_amd
    return seekstorm_amd


@pytest.fixture(scope="module")
def N():
    from seekstorm_amd import _native
    return _native


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


# ------------------------------------------------------------------------------------------------ the header's rule, restated
def _rule(budget, n_sub, n_lists):
    """include/seekstorm_hip.h: rows = budget / (n_sub * 768) - 1 (the zero row); all lists own one if that covers them; else the longest
    lists own the fixed rows and a quarter of the rows, none below 32, is the pool -> (kind, rows, fixed, pool)"""
    rows = budget // (n_sub * ROW_BYTES)
    rows = rows - 1 if rows else 0
    if rows == 0:
        return ("none", 0, 0, 0)
    if rows >= n_lists:
        return ("all", n_lists, n_lists, 0)
    pool = rows // 4 if rows >= 32 else 0
    return ("rationed", rows, rows - pool, pool)


def test_the_budget_walk_is_the_one_the_header_gives():
    """48 lists under B = 41 * 32 * 768 bytes at n_sub 16, 32, 35, 40: unrationed, 40 = 30 + 10, 36 = 27 + 9, 31 without a pool"""
    assert N_SUB == [16, 32, 35, 40]
    assert [_rule(BUDGET, n, 48) for n in N_SUB] == [("all", 48, 48, 0), ("rationed", 40, 30, 10), ("rationed", 36, 27, 9), ("rationed", 31, 31, 0)]
    assert [_rule(NO_INDEX, n, 48)[0] for n in N_SUB] == ["none"] * 4


# ------------------------------------------------------------------------------------------------ corpora
def _planted_matches(terms, words, field=None):
    """docs (of any field, or of `field`) in which the words stand at consecutive positions"""
    n = 0
    for (d, f), ps in terms[words[0]].items():
        if field is not None and f != field:
            continue
        n += any(all(p + i in terms[w].get((d, f), ()) for i, w in enumerate(words)) for p in ps)
    return n


def _place_edges(terms, edge_lists, field_of=lambda i: 0):
    for t in edge_lists:
        for key in [k for k in terms[t] if k[0] >> 12 == LONE_SB]:
            del terms[t][key]
        terms[t][(LONE_SB * 4096 + 777, field_of(0))] = [5]
        for i, d in enumerate(EDGE_DOCS):
            terms[t].setdefault((d, field_of(i)), [3, 9])
    for key in [k for k in terms[edge_lists[0]] if k[0] >> 12 == HOLE_SB]:
        del terms[edge_lists[0]][key]


def _build_a(O):
    rng = np.random.default_rng(41)
    dl = O.lex_doclen(N_DOCS)[None, :]
    base = iter(int(round(0.08 * N_DOCS * 0.8955 ** i)) for i in range(A_TERMS - 1))  # 12 886 .. 80
    ok_docs = np.array([d for d in range(N_DOCS) if d >> 12 not in (LONE_SB, HOLE_SB)])
    terms = []
    for t in range(A_TERMS):
        if t == A_EMPTY:
            terms.append({})
            continue
        n = next(base)
        if t == A_L2_ONLY:
            d = np.concatenate([2 * LVL + rng.choice(N_DOCS - 2 * LVL, n, replace=False), rng.choice(LVL, 3, replace=False)])
        else:
            d = rng.choice(N_DOCS, n, replace=False)
        tf = np.minimum(rng.geometric(0.5, len(d)), 8)
        pos = rng.integers(0, 30, len(d))[:, None] + np.cumsum(rng.integers(2, 5, (len(d), 8)), axis=1)  # gaps >= 2: no chance phrase inside a list
        terms.append({(int(dd), 0): pos[j, :tf[j]].tolist() for j, dd in enumerate(d)})
    terms[A_ABSENT_L1] = {k: v for k, v in terms[A_ABSENT_L1].items() if not LVL <= k[0] < 2 * LVL}
    for words, nd in A_PLANT:
        for d in rng.choice(ok_docs, nd, replace=False):
            st = 100 + int(rng.integers(0, 40))
            for i, w in enumerate(words):
                e = terms[w].setdefault((int(d), 0), [])
                e.append(st + i)
    _place_edges(terms, A_EDGE)
    o, d, f, tf, ps = [0], [], [], [], []
    for e in terms:
        for key in sorted(e):
            p = sorted(set(e[key]))
            d.append(key[0]); f.append(0); tf.append(len(p)); ps += p
        o.append(len(d))
    c = Corpus(dl, np.asarray(o, np.uint64), np.asarray(d, np.uint32), np.asarray(f, np.uint8), np.asarray(tf, np.uint16), np.asarray(ps, np.uint16))
    c.planted = {tuple(w): _planted_matches(terms, w) for w, _ in A_PLANT}
    return c


def _build_b(O):
    from test_gpu_phrase import _corpus_fields
    dl, offs, docs, fields, tfs, positions = _corpus_fields(O, N_DOCS, 3, B_DFS, 31, B_PLANT, B_CROSS)
    planted = {}

    def edit(terms):
        terms[B_ABSENT_L1] = {k: v for k, v in terms[B_ABSENT_L1].items() if not LVL <= k[0] < 2 * LVL}
        _place_edges(terms, B_EDGE, lambda i: i % 3)
        for words, f, _ in B_PLANT:
            planted[(tuple(words), f)] = _planted_matches(terms, words, f)

    c = Corpus(dl, *_edit(offs, docs, fields, tfs, positions, edit))
    c.planted = planted
    return c


class World:
    """a corpus, how it is committed and uploaded, and which lists the header's rule gives rows at every step"""

    def __init__(self, c, n_terms, n_dense, budget):
        self.c, self.nt, self.nd, self.budget = c, n_terms, n_dense, budget
        self.RF = c.dl.shape[0]
        self.L = 1 if self.RF == 1 else self.RF + 1  # lists per term: the fields' and the merged one (virtual list t * L + f)
        self.tier = n_dense < n_terms
        self._vdf = {}

    def vdf(self, i):
        """posting counts of the dense terms' virtual lists over the prefix of step i"""
        if i not in self._vdf:
            c, hi = self.c, STEPS[i][2]
            m = (c.docs < hi) & (c.eterm < self.nd)
            t, d, f = c.eterm[m].astype(np.int64), c.docs[m].astype(np.int64), c.fields[m].astype(np.int64)
            out = np.zeros((self.nd, self.L), np.int64)
            if self.L == 1:
                out[:, 0] = np.bincount(t, minlength=self.nd)
            else:
                out[:, :self.RF] = np.bincount(t * self.RF + f, minlength=self.nd * self.RF).reshape(self.nd, self.RF)
                out[:, self.RF] = np.bincount(np.unique(t * (1 << 32) + d) >> 32, minlength=self.nd)  # the merged list: every doc once
            self._vdf[i] = out.reshape(-1)
        return self._vdf[i]

    def rule(self, i):
        return _rule(self.budget, N_SUB[i], self.nd * self.L)

    def lists_rowed(self, i):
        """per virtual list: owns a fixed row (the longest lists first) or, empty, reads the zero row"""
        kind, _, fixed, _ = self.rule(i)
        df = self.vdf(i)
        if kind == "none":
            return np.zeros(len(df), bool)
        if kind == "all":
            return np.ones(len(df), bool)
        order = np.argsort(-df, kind="stable")
        assert df[order[fixed - 1]] > df[order[fixed]], "a tie at the last fixed row: the rule does not say who owns it"
        has = np.zeros(len(df), bool)
        has[order[:fixed]] = True
        return has | (df == 0)

    def terms_probed(self, i):
        return self.lists_rowed(i).reshape(self.nd, self.L).all(axis=1)

    def rank(self, i, t):
        """place of (single-field) list t among the lists by df at step i"""
        return int(np.nonzero(np.argsort(-self.vdf(i), kind="stable") == t)[0][0])

    def _split(self, cut):
        dl, o, d, f, t, p = cut
        e = int(o[self.nd])
        pe = int(t[:e].astype(np.int64).sum())
        return dl, (o[:self.nd + 1], d[:e], f[:e], t[:e], p[:pe]), (o[self.nd:] - o[self.nd], d[e:], f[e:], t[e:], p[pe:])

    def commit(self, sh, i):
        lv, lo, hi = STEPS[i]
        dl, o, d, f, t, p = self.c.level(lo, hi, self.nt)
        if self.RF == 1:  # ss_bm25_append_level_positions (+ ss_bm25_append_sparse_level)
            sh.commit_level(lv, dl[0], o, d, t, n_dense_terms=self.nd if self.tier else None, positions=p)
        elif self.tier:   # ss_bm25_commit_level_fields + ss_bm25_commit_sparse_level_fields
            sh.commit_level_fields_tiered(lv, dl, BOOST, o, d, f, t, self.nd, positions=p)
        else:
            sh.commit_level_fields(lv, dl, BOOST, o, d, f, t, positions=p)

    def upload(self, sh, i):
        hi = STEPS[i][2]
        dl, dense, rare = self._split(self.c.prefix(hi, self.nt))
        if self.RF == 1:
            sh.upload_lexical(hi, dl[0], dense[0], dense[1], dense[3], dense[4])
            if self.tier:
                assert sh.append_sparse(rare[0], rare[1], rare[3], positions=rare[4]) == self.nd
        else:
            sh.upload_lexical_fields(hi, dl, BOOST, *dense)
            if self.tier:
                assert sh.append_sparse_fields(*rare[:4], positions=rare[4]) == self.nd


def _check_edges(c, edge_lists):
    of = lambda t: c.docs[int(c.offs[t]):int(c.offs[t + 1])]
    for t in edge_lists:
        for d in EDGE_DOCS:
            assert d in of(t), (t, d)
        assert np.sum(of(t) >> 12 == LONE_SB) == 1, t
    assert np.sum(of(edge_lists[0]) >> 12 == HOLE_SB) == 0  # a (term, sub-block) cell of a rowed list that the fill must write as zeros


@pytest.fixture(scope="module")
def corpus_a(O):
    c = _build_a(O)
    w = World(c, A_TERMS, A_TERMS, BUDGET)
    # what the corpus must hold, so that nothing below passes vacuously
    assert c.offs[A_EMPTY] == c.offs[A_EMPTY + 1]
    _check_edges(c, A_EDGE)
    assert [w.rule(i) for i in range(4)] == [("all", 48, 48, 0), ("rationed", 40, 30, 10), ("rationed", 36, 27, 9), ("rationed", 31, 31, 0)]
    for i in (1, 2, 3):
        has = w.lists_rowed(i)
        assert has[A_BIG].all() and has[A_EDGE[0]] and not has[A_EDGE[1]] and not has[A_EDGE[2]], i
        assert not has[[t for ph in A_SHORT_PHRASES for t in ph]].any(), i
    tw = World(c, A_TERMS, A_DENSE_TIERED, BUDGET)
    assert [tw.rule(i)[0] for i in range(4)] == ["all", "all", "rationed", "rationed"] and tw.rule(2)[3] == 9 and tw.rule(3)[3] == 0
    for i in (2, 3):
        assert tw.lists_rowed(i)[A_BIG].all() and not tw.lists_rowed(i)[A_EDGE[1]] and not tw.lists_rowed(i)[[36, 37]].any()
    assert w.vdf(1)[A_ABSENT_L1] == w.vdf(0)[A_ABSENT_L1] > 0 and w.rank(0, A_ABSENT_L1) != w.rank(1, A_ABSENT_L1)
    assert w.vdf(1)[A_L2_ONLY] == 3 and not w.lists_rowed(1)[A_L2_ONLY] and w.lists_rowed(3)[A_L2_ONLY]
    assert w.rank(1, A_L2_ONLY) > w.rank(2, A_L2_ONLY) > w.rank(3, A_L2_ONLY)
    assert len(set(tuple(w.lists_rowed(i)) for i in (1, 2, 3))) == 3  # the owners of the fixed rows change from commit to commit
    assert all(n >= 60 for n in c.planted.values()), c.planted
    return c


@pytest.fixture(scope="module")
def corpus_b(O):
    c = _build_b(O)
    w = World(c, B_TERMS, B_TERMS, BUDGET)
    assert c.offs[B_EMPTY] == c.offs[B_EMPTY + 1]
    _check_edges(c, B_EDGE)
    assert [w.rule(i) for i in range(4)] == [("all", 48, 48, 0), ("rationed", 40, 30, 10), ("rationed", 36, 27, 9), ("rationed", 31, 31, 0)]
    for i in (1, 2):  # a term whose merged list owns a fixed row while one of its field lists has none
        has = w.lists_rowed(i).reshape(B_TERMS, 4)
        assert any(has[t, 3] and not has[t, :3].all() for t in range(B_TERMS)), i
        assert has[0].all() and has[7, 3] and not has[7, :3].all() and not has[11].any() and w.vdf(i).reshape(B_TERMS, 4)[11].all(), i
    tw = World(c, B_TERMS, B_DENSE_TIERED, BUDGET_TIER_B)
    assert [tw.rule(i) for i in range(4)] == [("all", 36, 36, 0), ("rationed", 32, 24, 8), ("rationed", 29, 29, 0), ("rationed", 25, 25, 0)]
    assert all(n >= 60 for n in c.planted.values()), c.planted
    return c


# ------------------------------------------------------------------------------------------------ three shards side by side
def _dev_mask(q, vouch):
    """ops_mask of ss_bm25_search_dev for a batch of unions and intersections (include/seekstorm_hip.h): bits 0 / 1 the kinds, 8..15 the most
    terms with NOT terms, 16..23 without, 24..27 the most NOT terms, bit 2 the vouch "every term has probe rows" """
    np_max, nn_max = int(q["n_terms"].max()), int(((q["op"] >> 8) & 0xFF).max())
    # (a batch with NOT terms declares bits 8..15 > bits 16..23 even when its longest query has none)
    return 1 | 2 | (4 if vouch else 0) | ((np_max + nn_max) << 8) | (np_max << 16) | (nn_max << 24)


class Trio:
    def __init__(self, S, N, w, budget):
        self.S, self.N, self.w = S, N, w
        self.inc, self.one, self.full = S.Shard(0), S.Shard(0), S.Shard(0)
        self.inc.set_probe_budget(budget)
        self.one.set_probe_budget(budget)
        self.rationed = (self.inc, self.one)
        self.rec = np.zeros((N_DOCS, 2), np.uint8)
        self.rec[:, 0] = np.arange(N_DOCS) % 7

    def close(self):
        for sh in (self.inc, self.one, self.full):
            sh.close()

    def step(self, i):
        """the commit, the two uploads, and -- before any search -- the rows both builders dealt against the header's rule"""
        w, hi = self.w, STEPS[i][2]
        w.commit(self.inc, i)
        w.upload(self.one, i)
        w.upload(self.full, i)
        st_i, st_o = self.state(self.inc), self.state(self.one)
        want = w.terms_probed(i)
        assert np.array_equal(st_i, st_o), (i, st_i, st_o)
        assert np.array_equal(st_i != 0, want), (i, "rows dealt", np.nonzero(st_i)[0], "the header's rule", np.nonzero(want)[0])
        assert not (st_i == 2).any(), (i, "a pool row survived the commit", st_i)
        assert (self.state(self.full) == 1).all()
        assert np.array_equal(self.inc.posting_count(np.arange(w.nt)), self.full.posting_count(np.arange(w.nt)))
        for sh in (self.inc, self.one, self.full):
            sh.upload_facets(self.rec[:hi])
        return st_i

    def state(self, sh, terms=None):
        """ss_bm25_term_probed: 0 = some list without a row, 1 = all lists rowed, 2 = one of them a pool row; 3 = a term of the sparse tier"""
        t = np.arange(self.w.nd) if terms is None else np.asarray(terms, np.int64)
        out = np.full(len(t), 3, np.uint8)
        dense = np.ascontiguousarray(t[t < self.w.nd], np.uint32)
        got = np.zeros(len(dense), np.uint8)
        if len(dense):
            self.N.check(self.N.lib().ss_bm25_term_probed(sh._h, len(dense), self.N.ptr(dense, self.N.u32p), self.N.ptr(got, self.N.u8p)), "ss_bm25_term_probed")
        out[t < self.w.nd] = got
        return out

    def states(self, terms):
        """... on inc, which one must match"""
        a, b = self.state(self.inc, terms), self.state(self.one, terms)
        assert np.array_equal(a, b), (terms, a, b)
        return a

    def answer(self, sh, q, k, rt):
        try:
            return tuple(np.copy(x) for x in sh.search_lexical_batch(q, k, rt, reference_shortcuts=False))
        except self.N.SeekStormHipError as e:
            return ("refused", e.code)

    def ask(self, tl, qt, k, rt, nots=None, ff=None, what=None):
        """one batch on the three shards: inc and one answer like full, every output array -> full's answer.  No shape of this module is
        refused by the unrationed shard, so a refusal is never accepted in place of an answer"""
        qs = [sh.make_queries(tl, qt, nots, field_filter=ff) for sh in (self.full, self.inc, self.one)]
        for q in qs[1:]:
            assert np.array_equal(q.view(np.uint8), qs[0].view(np.uint8)), ("idf differs: the images disagree on N or df", what)
        ref, a, b = (self.answer(sh, q, k, rt) for sh, q in zip((self.full, self.inc, self.one), qs))
        what = (what, [list(x) for x in tl], None if nots is None else [list(x) for x in nots], ff, int(k), int(rt), str(qt))
        assert not isinstance(ref[0], str), ("the unrationed shard refused", ref, what)
        for name, got in (("inc", a), ("one", b)):
            assert not isinstance(got[0], str), (name, "refused what the unrationed shard answers", got, what)
            for field, x, y in zip(("docs", "scores", "counts", "totals"), got, ref):
                assert np.array_equal(x, y), (name, field, what, np.nonzero(np.atleast_1d((x != y).reshape(len(x), -1).any(axis=1)))[0])
        return ref

    def sets(self, tl, nots=None, ff=None, what=None, ks=(10, 100), qts=None, rts=None):
        S = self.S
        out = {}
        for qt in qts or (S.QueryType.Union, S.QueryType.Intersection):
            for k in ks:
                for rt in rts or (S.ResultType.Topk, S.ResultType.TopkCount, S.ResultType.Count):
                    out[(qt, k, rt)] = self.ask(tl, qt, k, rt, nots, ff, what)
        return out

    def phrases(self, phrases, ff=None, min_total=None, what=None, ks=(10, 100)):
        """inc's answers equal full's; an empty success is never accepted where a phrase was planted"""
        S = self.S
        for k in ks:
            for rt in (S.ResultType.TopkCount, S.ResultType.Count):
                ref = self.ask(phrases, S.QueryType.Phrase, k, rt, ff=ff, what=what)
                for ph, n in (min_total or {}).items():
                    assert int(ref[3][phrases.index(list(ph))]) >= n, (what, ph, ff, ref[3])

    def launches(self, tl, qt, k, rt, nots=None, what=None):
        """... and how many search launches the rationed shards needed for the batch (profile slot 0, as tests/test_gpu_pruned.py reads it)"""
        for sh in self.rationed:
            sh.profile(True)
            sh.profile_read(0, reset=True)
        self.ask(tl, qt, k, rt, nots, what=what)
        n = [sh.profile_read(0, reset=True)[0] for sh in self.rationed]
        for sh in self.rationed:
            sh.profile(False)
        assert n[0] == n[1], (what, n)
        return n[0]

    def delete(self, hi):
        gone = [] if hi is None else np.unique(np.concatenate([np.arange(0, hi, 64), np.arange(63, hi, 64), [hi - 1]])).astype(np.uint64)
        for sh in (self.inc, self.one, self.full):
            sh.set_deleted(gone)
        return gone

    def facets(self, tl, what):
        """facet counts over the match set of a union: equal to full's -- or, where a dense list has no row and no pool can give it one, refused
        with SS_ENOTSUP (the code tests/test_gpu_tier_facets.py pins) by inc and one alike -> answered?"""
        S, N = self.S, self.N
        ref = self.full.facet_count(self.full.make_queries(tl, S.QueryType.Union), 0, "string16", n_buckets=7)
        assert ref[2] > 0 and int(ref[0].sum()) == ref[2], (what, ref)
        got = []
        for sh in self.rationed:
            try:
                r = sh.facet_count(sh.make_queries(tl, S.QueryType.Union), 0, "string16", n_buckets=7)
                assert np.array_equal(r[0], ref[0]) and r[1:] == ref[1:], (what, r, ref)
                got.append(True)
            except N.SeekStormHipError as e:
                assert e.code == N.SS_ENOTSUP, (what, e.code)
                got.append(False)
        assert got[0] == got[1], (what, got)
        return got[0]


def _pairs(lists, partners):
    return [[int(t), int(partners[j % len(partners)])] for j, t in enumerate(lists)]


def _differs(got, ref, rt_count):
    """answers of the device-pointer entry against the host-pointer entry's: the rows up to each query's count"""
    if not np.array_equal(got[2], ref[2]) or (rt_count and not np.array_equal(got[3], ref[3])):
        return "counts"
    for i in range(len(got[2])):
        c = int(got[2][i])
        if not (np.array_equal(got[0][i][:c], ref[0][i][:c]) and np.array_equal(got[1][i][:c], ref[1][i][:c])):
            return "query %d" % i
    return None


# ------------------------------------------------------------------------------------------------ worlds A and C-A: one indexed field
def _fill_pool(T, rowless, pool, big):
    """name `pool` row-less lists: afterwards each of them holds a pool row (ss_bm25_term_probed: 2), on inc and on one"""
    S = T.S
    chosen = [int(t) for t in rowless[:pool]]
    T.ask(_pairs(chosen, big), S.QueryType.Union, 10, S.ResultType.TopkCount, what="fill the pool")
    assert (T.states(chosen) == 2).all(), T.states(chosen)
    return chosen


def _step_single_field(T, O, i, carried):
    """everything world A asks of one step; -> the lists that hold pool rows when the step ends (the next commit must forget them)"""
    S, N, w = T.S, T.N, T.w
    hi = STEPS[i][2]
    fresh = T.step(i)
    kind, rows, fixed, pool = w.rule(i)
    df = w.vdf(i)
    rowed = [t for t in range(w.nd) if fresh[t] == 1 and df[t] > 0]
    rowless = [t for t in A_EDGE if t < w.nd and fresh[t] == 0] + [t for t in range(w.nd) if fresh[t] == 0 and t not in A_EDGE]
    assert (kind == "all") == (not rowless) and (kind == "none") == (not rowed)
    big = A_BIG
    U, I = S.QueryType.Union, S.QueryType.Intersection
    TOPK, TC, CNT = S.ResultType.Topk, S.ResultType.TopkCount, S.ResultType.Count

    # rows across the swap: the lists that held pool rows before the commit mean nothing now -- the first batch naming them answers like full
    if carried:
        if kind == "rationed":
            assert (fresh[carried] == 0).any(), (i, carried, fresh[carried])
        T.ask(_pairs(carried, big) + [carried[:3] + [3]], U, 10, TC, what=(i, "first batch after the swap"))
        T.ask(_pairs(carried, big), I, 10, TC, what=(i, "first batch after the swap"))

    # all lists rowed
    if rowed:
        l2 = A_L2_ONLY if A_L2_ONLY in rowed else 4
        tl = [[0], [3], [0, 1], [3, 5, 1], [0, 1, 2, 3], [2, 4], [3, l2], [1, A_EMPTY], [l2, 0, 3], [5]]
        nots = [[], [], [5], [], [], [3], [], [], [1], [3, 0]]
        assert (T.states(sorted({t for q in tl + nots for t in q})) == 1).all()
        ref = T.sets(tl, nots, what=(i, "rowed lists"))
        # (batches this small take the one-launch kernel: the staged pruned kernels read the same fixed rows through the device-pointer entry)
        from test_gpu_device_entry import _dev_search
        for qt in (U, I):
            for sh in T.rationed:
                q = sh.make_queries(tl, qt, nots)
                assert _differs(_dev_search(S, sh, q, 10, TC, _dev_mask(q, True)), ref[(qt, 10, TC)], True) is None, (i, qt, "staged, rowed lists")
        T.delete(hi)
        T.sets(tl, nots, what=(i, "rowed lists, tombstones"), ks=(10,))
        T.delete(None)

    # row-less lists <= pool: built on demand, one launch, nothing left to the scans
    if pool:
        chosen = rowless[:pool]
        assert set(chosen) >= {t for t in A_EDGE[1:] if t < w.nd} and len(chosen) == pool
        tl = _pairs(chosen[:-1], big) + [[chosen[0], chosen[1], 3], [0, 1], [chosen[2], 3, 5, 1]]
        nots = [[] for _ in chosen[:-1]] + [[], [chosen[-1]], [0]]
        st = T.states(chosen)
        assert (st != 1).all() and (st == 0).any(), st  # row-less (or holding a pool row since the batch after the swap)
        assert T.launches(tl, U, 10, TOPK, nots, what=(i, "row-less lists <= pool")) == 1
        assert (T.states(chosen) == 2).all()
        T.sets(tl, nots, what=(i, "row-less lists <= pool"))
        assert (T.states(chosen) == 2).all()

        # eviction and return: X gets a row, `pool` other row-less lists take every row of the pool, X gets one again
        x = chosen[0]
        others = [t for t in rowless if t != x][:pool]
        assert len(others) == pool
        assert T.states([x])[0] == 2
        T.ask(_pairs(others, big), U, 10, TC, what=(i, "evict X"))
        assert T.states([x])[0] == 0 and (T.states(others) == 2).all()
        # (facet counts read the match set from the bit records: the row-less list gets a row again, over the planted edge docs)
        assert T.facets([[3, x]], (i, "facets, a row-less list beside a pool")) and T.states([x])[0] == 2
        T.ask(_pairs(others[:pool - 1], big), I, 10, TC, what=(i, "evict X"))
        T.ask(_pairs(others[-1:], big), I, 10, TC, what=(i, "evict X"))
        assert T.states([x])[0] == 0
        T.ask([[x, 3], [x], [x, 0, 1]], U, 100, TC, [[], [], [others[0]]], what=(i, "X again"))
        assert T.states([x])[0] == 2

        # row-less lists > pool: a mixed batch, run as two
        assert len(rowless) > pool
        tl = _pairs(rowless, big) + [[0, 1], [3, 2], [4, 5]]
        assert T.launches(tl, U, 10, TC, what=(i, "more row-less lists than pool rows")) == 2
        for qt, rt in ((I, TC), (U, TOPK), (I, CNT)):
            T.ask(tl, qt, 10, rt, what=(i, "more row-less lists than pool rows"))
        T.delete(hi)
        T.sets(tl, what=(i, "more row-less lists than pool rows, tombstones"), ks=(10,), rts=(TC,))
        T.delete(None)

    # rationed without a pool, or no index at all: a batch naming row-less lists scans
    if rowless and not pool:
        tl = _pairs(rowless[:12], big) + [[rowless[0], rowless[1]], [rowless[2]], [0, 1]]
        nots = [[] for _ in rowless[:12]] + [[], [rowless[3]], [rowless[4]]]
        assert (T.states(rowless) == 0).all()
        before = [sh.one_launch_batches() for sh in T.rationed]
        T.sets(tl, nots, what=(i, "row-less lists, no pool"))
        T.delete(hi)
        T.sets(tl, nots, what=(i, "row-less lists, no pool, tombstones"), ks=(10,))
        T.delete(None)
        assert (T.states(rowless) == 0).all() and [sh.one_launch_batches() for sh in T.rationed] == before
        for sh in T.rationed:  # forced PRUNED: refused, not answered some other way
            sh.set_strategy(N.BM25_PRUNED)
            try:
                assert T.answer(sh, sh.make_queries(tl[:3], U), 10, TOPK) == ("refused", N.SS_ENOTSUP)
            finally:
                sh.set_strategy(N.BM25_AUTO)
        # facet counts: the row-less list cannot get a row -> SS_ENOTSUP, on both; rowed lists are counted
        assert not T.facets([[3, rowless[0]]], (i, "facets, a row-less list and no pool"))
        if rowed:
            assert T.facets([[3, 0]], (i, "facets, rowed lists"))

    # wider and deeper: unions of 7 and 8 lists (the scans, rows or not), k = 300
    tail = [t for t in (34, 36, 37, 30, 20) if t < w.nd]
    T.sets([[0, 3] + tail, [0, 1, 2, 3, 4, 34, 35, 38]], what=(i, "unions of 7 and 8 lists"), ks=(10,), qts=(U,), rts=(TC, TOPK))
    T.sets([[0, 34], [3, 1, 36], [A_L2_ONLY, 35]], what=(i, "k = 300"), ks=(300,), rts=(TC,))

    # phrases: over rowed lists, over row-less lists (beside a pool and without one), the 7-term phrase of the generic kernel
    planted = {tuple(ph): 10 for ph, _ in A_PLANT}
    if kind == "rationed":
        st = T.states([t for ph in A_SHORT_PHRASES for t in ph])
        assert ((st == 0) | (st == 2) | (st == 3)).all(), st
    T.phrases(A_PHRASES, min_total=planted, what=(i, "phrases"))
    T.delete(hi)
    T.phrases(A_PHRASES, what=(i, "phrases, tombstones"), ks=(10,))
    T.delete(None)

    # the sparse tier on top: rowed dense, row-less dense and sparse terms in one query; k <= 32 one launch, k = 100 the staged tiered pipeline
    if w.tier:
        mid = rowless[0] if rowless else 34
        tl = [[0, 45], [mid, 46], [3, mid, 41], [36, 47, 1], [44], [35, 40, 0, 2], [44, 3], [45, 46]]
        nots = [[], [], [5], [], [], [], [mid], [0]]
        before = T.inc.one_launch_batches()
        T.sets(tl, nots, what=(i, "both tiers"), ks=(10, 32), rts=(TC, TOPK))
        if kind == "all" or pool:
            assert T.inc.one_launch_batches() >= before + 8, (i, "the one-launch path did not take the tiered batches")
        T.sets(tl, nots, what=(i, "both tiers"), ks=(100,), rts=(TC, TOPK))
        T.phrases([[45, 46], [2, 40], [36, 37, 45]], min_total={(45, 46): 10, (2, 40): 10, (36, 37, 45): 10}, what=(i, "phrases, both tiers"), ks=(10,))
        T.delete(hi)
        T.sets(tl, nots, what=(i, "both tiers, tombstones"), ks=(10, 100), rts=(TC,))
        T.delete(None)

    # one launch against the staged pipeline (the device-pointer entry never takes the one-launch path), and the vouch of that entry
    if kind == "all" or pool:
        from test_gpu_device_entry import _dev_search
        chosen = _fill_pool(T, rowless, pool, big) if pool else []
        tl = _pairs(chosen, big) + [[0, 1], [3, 5, 1], [0, 1, 2, 3], [3]]
        nots = [[] for _ in chosen] + [[5], [], [], [4]]
        for qt in (U, I):
            before = [sh.one_launch_batches() for sh in T.rationed]
            ref = T.ask(tl, qt, 10, TC, nots, what=(i, "one launch"))
            assert [sh.one_launch_batches() for sh in T.rationed] == [b + 1 for b in before], (i, "the one-launch kernel did not run")
            for sh in T.rationed:
                q = sh.make_queries(tl, qt, nots)
                for vouch in (False, True):  # (the vouch holds: every list of the batch has a row at this moment)
                    assert _differs(_dev_search(S, sh, q, 10, TC, _dev_mask(q, vouch)), ref, True) is None, (i, qt, vouch, "staged != one launch")
        if pool:  # a vouch gone stale: X loses its row to host-pointer batches over other lists; the same device call reports X's query, only it
            x = chosen[0]
            tl = [[x, 0], [3, 1], [x], [0, 1, 2]]
            refs = {sh: T.answer(T.full, T.full.make_queries(tl, U), 10, TC) for sh in T.rationed}
            held = {}
            assert T.states([x])[0] == 2
            for sh in T.rationed:
                q = sh.make_queries(tl, U)
                held[sh] = _dev_search(S, sh, q, 10, TC, _dev_mask(q, True))
                assert _differs(held[sh], refs[sh], True) is None, (i, "a vouch that holds")
            others = [t for t in rowless if t != x][:pool]
            T.ask(_pairs(others, big), U, 10, TC, what=(i, "evict X under the vouch"))
            assert T.states([x])[0] == 0
            for sh in T.rationed:
                q = sh.make_queries(tl, U)
                doc, score, cnt, tot = _dev_search(S, sh, q, 10, TC, _dev_mask(q, True))
                for j in (0, 2):
                    assert cnt[j] == BAD and (doc[j] == BAD).all() and tot[j] == 0, (i, j, cnt, tot)
                for j in (1, 3):
                    c = int(cnt[j])
                    assert c == held[sh][2][j] and tot[j] == held[sh][3][j]
                    assert np.array_equal(doc[j][:c], held[sh][0][j][:c]) and np.array_equal(score[j][:c], held[sh][1][j][:c])
            T.ask(tl, U, 10, TC, what=(i, "after the stale vouch"))  # (and the host-pointer entry gives X its row back)

    # the CPU oracle, at the last step: a list that had no row when the step began in every query
    if i == len(STEPS) - 1:
        c = w.c
        osh = O.Shard(N_DOCS, c.dl[0], c.offs, c.docs, c.tfs)
        osh.set_positions(c.positions)
        if kind != "all":
            assert fresh[34] == 0 and fresh[36] == 0 and fresh[37] == 0
        for terms, qt, op in (([0, 34], U, O.OP_OR), ([3, 34], I, O.OP_AND), ([36, 44, 1], U, O.OP_OR)):
            doc, score, cnt, tot = T.ask([terms], qt, 10, TC, what="oracle")
            od, os_, otot = osh.search_exhaustive(terms, op, 10)
            assert otot > 0 and int(tot[0]) == otot and int(cnt[0]) == len(od) and np.allclose(score[0][:len(od)], os_, rtol=1e-4), terms
        doc, score, cnt, tot = T.ask([[36, 37, 45]], S.QueryType.Phrase, 10, TC, what="oracle")
        od, os_, otot = osh.search_phrase([36, 37, 45], [0, 1, 2], 10)
        assert otot >= 10 and int(tot[0]) == otot and int(cnt[0]) == len(od) and np.allclose(score[0][:len(od)], os_, rtol=1e-4)

    # leave the pool full of rows: the next commit must forget every one of them
    return _fill_pool(T, rowless[::-1], pool, big) if pool else []


def _walk(T, O, step_fn):
    try:
        carried = []
        for i in range(len(STEPS)):
            carried = step_fn(T, O, i, carried)
            assert T.inc.incremental_info()[0] == STEPS[i][0] + 1
    finally:
        T.close()


def test_world_a_one_field_four_commits_one_budget(S, N, O, corpus_a):
    """World A.  ss_bm25_append_level_positions under one byte budget: 48 rows, 30 + 10, 27 + 9, 31 + 0.  Per step: the rows dealt (inc == one ==
    the header's rule), the batch after the swap, all-rowed / <= pool / > pool (two launches) / no-pool batches of unions and intersections
    with NOT terms at k 10 and 100 in the three result types, unions of 7 and 8 lists, k = 300, phrases over rowed and row-less lists and the
    7-term phrase, tombstones on the planted edge docs, eviction and return (2 -> 0 -> 2), facet counts, one launch against the staged
    pipeline, the vouch of ss_bm25_search_dev kept and gone stale; the oracle at the last step."""
    _walk(Trio(S, N, World(corpus_a, A_TERMS, A_TERMS, BUDGET), BUDGET), O, _step_single_field)


def test_world_a_without_a_probe_index(S, N, O, corpus_a):
    """The same commits under a budget below two rows' bytes: max_rows == 0, no probe index at any step.  terms_probed is all false, forced
    BM25_PRUNED is refused with SS_ENOTSUP, and every query -- phrases included, which then take the generic kernel -- is answered like full."""
    _walk(Trio(S, N, World(corpus_a, A_TERMS, A_TERMS, NO_INDEX), NO_INDEX), O, _step_single_field)


def test_world_c_one_field_with_a_sparse_tier(S, N, O, corpus_a):
    """World C over world A's corpus: the last 8 lists as a sparse tier (commit_level(n_dense_terms=40): ss_bm25_append_level_positions +
    ss_bm25_append_sparse_level), 40 dense lists under the same budget: unrationed twice, 27 + 9, 31 + 0.  World A's checks over the dense
    lists, and queries mixing rowed dense, row-less dense and sparse terms at k 10 / 32 (one launch) and 100 (staged tiered pipeline)."""
    _walk(Trio(S, N, World(corpus_a, A_TERMS, A_DENSE_TIERED, BUDGET), BUDGET), O, _step_single_field)


# ------------------------------------------------------------------------------------------------ worlds B and C-B: three indexed fields
B_SETS = [[0, 1], [1, 2, 3], [6, 7], [0, 7], [9, 10], [7, 9, 10, 0], [10], [7, 6], [5, 0], [8, 0], [4, 6], [11, 0], [6, 9, 10]]
B_NOTS = [[], [4], [], [], [], [], [], [0], [], [], [10], [], [1]]
# (intersections under a filter: pairs that co-occur in one of the listed fields, planted there where the dfs are too small for chance)
B_FILTERED = {(1,): [[0, 1], [7, 6], [9, 10], [0, 7], [6, 10], [10], [7], [11, 7]],
              (0, 2): [[0, 1], [7, 6], [9, 10], [0, 7], [6, 10], [10], [7], [11, 0], [6, 9, 10]]}
B_FILTERED_UNIONS = [[0, 1], [7, 6, 9], [0, 3, 6, 9, 10], [1, 2, 4, 5, 7, 6, 10]]


def _step_fields(T, O, i, carried):
    """everything world B asks of one step; -> the terms whose lists hold pool rows when the step ends"""
    S, N, w = T.S, T.N, T.w
    hi = STEPS[i][2]
    fresh = T.step(i)
    kind, rows, fixed, pool = w.rule(i)
    has = w.lists_rowed(i).reshape(w.nd, 4)
    U, I = S.QueryType.Union, S.QueryType.Intersection
    TOPK, TC, CNT = S.ResultType.Topk, S.ResultType.TopkCount, S.ResultType.Count
    sets, nots = B_SETS, B_NOTS
    merged_less = [t for t in range(w.nd) if not has[t, 3]]              # terms whose merged list has no row
    field_less = [t for t in range(w.nd) if has[t, 3] and not has[t, :3].all()]  # ... whose merged list has one and some field list has none

    if carried:  # the terms that held pool rows before the commit: without a filter (merged lists) and with one (field lists)
        T.ask(_pairs(carried, [0, 1]), U, 10, TC, what=(i, "first batch after the swap"))
        T.ask(_pairs(carried, [0, 1]), I, 10, TC, ff=(1,), what=(i, "first batch after the swap"))

    # without a filter: the merged lists
    if kind == "rationed":
        assert merged_less or field_less
        assert (T.states(merged_less + field_less) != 1).all()
        if pool:
            assert field_less, (i, "no term with a rowed merged list over a row-less field list")
    T.sets(sets, nots, what=(i, "merged lists"))
    # under a filter: intersections read the field lists and so need other rows
    for ff in ((1,), (0, 2)):
        if kind == "rationed":
            st = T.states(field_less + merged_less)
            assert (st != 1).all(), (i, ff, st)
        res = T.sets(B_FILTERED[ff], ff=ff, what=(i, "filtered intersections", ff), qts=(I,), rts=(TC, CNT))
        assert (res[(I, 10, TC)][3] > 0).all(), (i, ff, res[(I, 10, TC)][3])
        res = T.sets(B_FILTERED_UNIONS, ff=ff, what=(i, "filtered unions", ff), qts=(U,), rts=(TC, TOPK))
        assert (res[(U, 10, TC)][3] > 0).all(), (i, ff, res[(U, 10, TC)][3])
    # phrases always read the merged lists; a filter is a test on the positions' field tags
    T.phrases(B_PHRASES, min_total={tuple(ph): 10 for ph in B_PHRASES if ph != [1, 0]}, what=(i, "phrases"))
    for ff, phs in B_PHRASES_IN.items():
        T.phrases(phs, ff=ff, min_total={tuple(ph): 10 for ph in phs}, what=(i, "phrases", ff), ks=(10,))
    T.delete(hi)
    T.sets(sets, nots, what=(i, "merged lists, tombstones"), ks=(10,), rts=(TC,))
    T.sets(B_FILTERED[(1,)], ff=(1,), what=(i, "filtered intersections, tombstones"), ks=(10,), qts=(I,), rts=(TC,))
    T.sets(B_FILTERED_UNIONS, ff=(0, 2), what=(i, "filtered unions, tombstones"), ks=(10,), qts=(U,), rts=(TC,))
    T.phrases(B_PHRASES, what=(i, "phrases, tombstones"), ks=(10,))
    T.delete(None)

    if w.tier:  # terms 9, 10, 11 are sparse: one launch at k <= 32, the staged tiered pipeline at k = 100 (and for `sets` above, whose
        # union under a sparse NOT list is outside the one-launch shape)
        tl = [[0, 9], [7, 10], [6, 11, 1], [10], [5, 9, 0, 2], [9, 10], [7, 6]]
        tn = [[], [], [3], [], [], [0], []]
        before = T.inc.one_launch_batches()
        T.sets(tl, tn, what=(i, "both tiers"), ks=(10, 32), rts=(TC, TOPK))
        if kind == "all" or pool:
            assert T.inc.one_launch_batches() >= before + 8, (i, "the one-launch path did not take the tiered batches")
        T.sets(tl, tn, what=(i, "both tiers"), ks=(100,), rts=(TC, TOPK))

    if i == len(STEPS) - 1:  # the oracle: a filtered intersection over field lists without rows, a union over a row-less merged list
        c = w.c
        pdl, po, pd, pf, pt, pp = c.prefix(N_DOCS, w.nt)
        if kind == "rationed" and not w.tier:
            assert not has[7, :3].all() and not has[11, 3]
        for terms, qt, op, ff in (([7, 6], I, O.OP_AND, (1,)), ([0, 11], U, O.OP_OR, ()), ([11, 7], I, O.OP_AND, (1,))):
            doc, score, cnt, tot = T.ask([terms], qt, 10, TC, ff=ff or None, what="oracle")
            od, os_, otot, _ = O.search_fields_exhaustive(N_DOCS, pdl, BOOST, po, pd, pf, pt, terms, op, 10, field_filter=ff)
            assert otot > 0 and int(tot[0]) == otot and int(cnt[0]) == len(od) and np.allclose(score[0][:len(od)], os_, rtol=1e-4), (terms, ff)

    if not pool:
        return []
    # leave the pool full: the shortest dense terms' merged lists, then field lists
    tail = [t for t in range(w.nd - 1, -1, -1) if not has[t].all() and w.vdf(i).reshape(w.nd, 4)[t].all()][:max(1, pool // 4)]
    T.ask(_pairs(tail, [0, 1]), U, 10, TC, what=(i, "fill the pool"))
    T.ask(_pairs(tail, [0, 1]), I, 10, TC, ff=(0, 1, 2), what=(i, "fill the pool"))
    assert (T.states(tail) == 2).all(), T.states(tail)
    return tail


def test_world_b_three_fields_device_commits(S, N, O, corpus_b):
    """World B.  ss_bm25_commit_level_fields with positions under the same budget walk over 48 virtual lists (t * 4 + f, the merged list
    last).  Unions and intersections over the merged lists, the same terms under field filters (1,) and (0, 2) -- field lists, other rows --,
    filtered unions of 2 .. 7 terms, phrases with and without a filter, tombstones; terms whose merged list owns a fixed row while a field
    list has none (asserted from the dfs); the oracle on filtered intersections at the last step."""
    _walk(Trio(S, N, World(corpus_b, B_TERMS, B_TERMS, BUDGET), BUDGET), O, _step_fields)


def test_world_c_three_fields_with_a_sparse_tier(S, N, O, corpus_b):
    """World C over world B's corpus: terms 9 .. 11 as a sparse tier (commit_level_fields_tiered: ss_bm25_commit_level_fields +
    ss_bm25_commit_sparse_level_fields), 36 dense virtual lists under 33 * 32 * 768 bytes: unrationed, 24 + 8, 29 + 0, 25 + 0.  (With 9 dense
    terms every merged list is among the longest 24 lists: the row-less lists are field lists, which the filtered intersections naming a
    sparse term beside terms 5 .. 7 read.)"""
    _walk(Trio(S, N, World(corpus_b, B_TERMS, B_DENSE_TIERED, BUDGET_TIER_B), BUDGET_TIER_B), O, _step_fields)


# ------------------------------------------------------------------------------------------------ the generator's builder
def test_generated_image_under_a_budget(S, N, O):
    """ss_bm25_synth writes probe rows while it generates the postings (lex_gen_kernel: only where the list owns a row): a generated image
    under a budget with a pool answers like the same image without one, over rowed lists, lists that get pool rows and lists left to the scans"""
    n_docs, n_terms = 150_000, 48
    th = O.term_thresholds(n_terms)
    full, part = S.Shard(0), S.Shard(0)
    try:
        n_sub = (n_docs + 4095) // 4096
        part.set_probe_budget(41 * n_sub * ROW_BYTES)
        for sh in (full, part):
            sh.synth_lexical(O.LEX_SEED, n_docs, th, O.len_table())
        terms = np.arange(n_terms)
        df = full.posting_count(terms).astype(np.int64)
        assert np.array_equal(df, part.posting_count(terms).astype(np.int64)) and (df > 0).all()
        probed = part.terms_probed(terms)
        order = np.argsort(-df, kind="stable")
        assert df[order[29]] > df[order[30]]
        assert _rule(41 * n_sub * ROW_BYTES, n_sub, n_terms) == ("rationed", 40, 30, 10)
        assert probed.sum() == 30 and probed[order[:30]].all() and full.terms_probed(terms).all()
        rowed, rowless = [int(t) for t in order[:30]], [int(t) for t in order[30:]]
        batches = [_pairs(rowed[:8], rowed[8:]) + [rowed[:4]], _pairs(rowless[:9], rowed) + [[rowless[0], rowless[1], rowed[0]]],
                   _pairs(rowless, rowed) + [rowed[:2]]]
        for tl in batches:
            for qt in (S.QueryType.Union, S.QueryType.Intersection):
                for rt in (S.ResultType.Topk, S.ResultType.TopkCount, S.ResultType.Count):
                    a = full.search_lexical_batch(full.make_queries(tl, qt), 10, rt, reference_shortcuts=False)
                    b = part.search_lexical_batch(part.make_queries(tl, qt), 10, rt, reference_shortcuts=False)
                    for x, y in zip(a, b):
                        assert np.array_equal(x, y), (tl, qt, rt)
    finally:
        full.close(); part.close()
