"""Tiered-image answers doc for doc: queries that name a sparse-tier term (bm25_sparse_kernel + sp_seed_kernel + bm25_tier_merge_kernel,
role 3 of the one-launch kernel, bm25_search_tiered_excl) against naive.bm25_exact -- the crate's f32 factors summed in float64 -- with
the checks of test_gpu_score_edges (_check: no doc twice, every doc a match, every score within 1e-4 of ITS exact score, the docs above
the k-th score's tie band the reference's, bit-equal groups in doc-id order; exact_ties: the very list of the reference).

Two small worlds (n_docs = 3 * 4096 + 37: three full sub-blocks and a partial one), one indexed field, the first `nd` lists uploaded as
the dense image and the rest appended as the sparse tier:
  A, determined ties.  One length byte, every tf 1: a weight is exactly 1.0, a score the sum of the idfs of the terms a doc holds.  Each
     sparse list S<L> has a dense partner D<L> of the same df (L = k - 1, k, k + 1 for every k in use): in their union sparse-only and
     dense-only docs tie bit for bit, so the top k must be the k lowest doc ids ACROSS the tiers -- which needs dense docs scoring exactly
     the seed (the sparse list's k-th score) -- and the docs holding both terms stand in both lists of the merge.  T<n> is the n lowest
     doc ids of DW1 & DW2, whose docs tie in [DW1, DW2]: in [T<n>, DW1, DW2] the dense part's top-k is k docs of the sparse list with
     partial scores (n > k), or all n of them beside k - n others (n < k) -- a CPU test counts them for every k.
  B, seams.  Two lengths, tf in {1, 2, 3} (one of six weights per doc: few distinct scores, many exact ties).  Sparse lists of 1, 63, 64, 65, 511,
     512, 513 and 1025 postings (the sparse kernel's 64-posting step, its 8 waves x 64 round, the 4-wave KPL = 16 instance), postings on
     docs 0, 63, 64, 4095, 4096, 8191, 8192 and n_docs - 1, X and Y adjacent in the tier's array with Y's first doc searched for in X
     (sp_find returns X's end: absent), two lists sharing most docs (a union scores a doc under the FIRST sparse list that holds it), dense
     lists whose (term, sub-block) segments are empty / one full 16-byte unit / a unit plus one posting and padding, probed by dense_find
     beyond their last posting and at local docs 0 and 4095; tombstones on the word and sub-block seams and on every third doc of a list.
The sparse tier is appended in two calls (B: Y opens the second one).  Besides the batches of one operator that _run_all sends, every query
of a world goes out in ONE shuffled call, which the library splits by shape and must answer in the caller's order.
The tests that are not marked gpu prove on the CPU (naive only) that the worlds hold what they are built for, and that _check rejects a
duplicated doc, a doc with its partial score and a tie broken the wrong way.

Routing, as the path counters show it (asserted below): a host-pointer call of <= 256 queries (bm25_search_direct_locked's
SM_H_QUERIES, not 64) hands every query that fits to the one-launch kernel -- for a query naming a sparse term that is k <= 32, <= 4
scored terms, no sparse NOT term in a union -- so the staged pipeline with seeds is reached by repeating the set beyond 256 queries
(k <= 32), by any call at k > 32 and under the exhaustive strategy.  A 9- or 12-term intersection with a sparse term is NOT the generic
galloping kernel's on an image with one indexed field (bm25_shape_of sends there only filtered / per-field / all_terms_frequent
shapes): the sparse kernel drives it, generic_batches() stays.  Images with several indexed fields -- bm25_gallop.hip over per-field
lists, and filtered queries naming a sparse term (the gate of bm25_sparse.hip) -- are tests/test_gpu_fields_edges.py's, against
naive.bm25f_exact."""
import types

import numpy as np
import pytest

from oracle import naive
from test_gpu_score_edges import REL, _check, _gen, _run_all   # (_gen makes the Corpus that _check and _run_all read)

N_DOCS = 3 * 4096 + 37
# every KPL instance of the sparse and merge kernels on both sides of its seam (64 | 65, 128 | 129, 256 | 257), a deep page beyond
# the 1024 keys of the largest, and 32 | 33: the last k at which the one-launch path takes a query that names a sparse term
KS = (1, 10, 32, 33, 64, 65, 128, 129, 256, 257, 1024, 1500)
SEAM = [0, 63, 64, 4095, 4096, 8191, 8192, N_DOCS - 1]
TOMB = [0, 63, 64, 4095, 4096, N_DOCS - 1]
ONE_LAUNCH_MAX_Q = 256   # queries of one host-pointer call the one-launch path takes
ONE_LAUNCH_MAX_K = 32    # ... for a query that names a sparse term
T_SIZES = (5, 12, 30, 60, 70, 120, 135, 250, 262, 1000, 1030, 1490, 1510)   # world A's T<n>: for every k > 1 one above k and one in [k / 2, k)


class World:
    def __init__(self, n_docs, doclen, dense, sparse, tf, seed, exact):
        """dense / sparse: {name: docs}, in the order of their term ids (dense first)"""
        self.names = list(dense) + list(sparse)
        self.nd = len(dense)
        self.id = {name: i for i, name in enumerate(self.names)}
        self.c = _gen(n_docs, doclen, [(np.asarray(d), tf) for d in list(dense.values()) + list(sparse.values())], seed)
        self.exact = exact
        self.ors, self.ands, self.wide = [], [], []   # (terms, op_and, nots)
        self.deleted = ()

    def q(self, terms, op_and=False, nots=()):
        return ([self.id[t] for t in terms], op_and, tuple(self.id[t] for t in nots))

    def docs(self, name):
        return self.c.lists[self.id[name]][0].astype(np.int64)

    def is_sparse(self, term):
        return term >= self.nd

    def all_queries(self):
        return self.ors + self.ands + self.wide


def _wide_lists(rng, n, core, dense, fractions):
    for i, f in enumerate(fractions):
        dense[f"G{i}"] = np.union1d(core, rng.choice(n, int(f * n), replace=False))


def _build_a():
    rng = np.random.default_rng(101)
    n = N_DOCS
    dl = np.full(n, naive.int_to_byte4(100), np.uint8)
    dense, sparse = {}, {}
    not_seam = np.setdiff1d(np.arange(n), SEAM)
    for L in sorted({x for k in KS for x in (k - 1, k, k + 1) if x >= 1}):
        b = 0 if L < 9 else min(L // 3, 40)          # docs that hold both terms
        m = 2 * L - b
        if L in (65, 257, 1025):                     # (postings on the word and sub-block seams)
            docs = np.union1d(SEAM, rng.choice(not_seam, m - len(SEAM), replace=False))
        else:
            docs = np.sort(rng.choice(n, m, replace=False))
        both = np.zeros(m, bool)
        if b:
            both[np.linspace(2, m - 1, b).astype(int)] = True
        single = np.nonzero(~both)[0]                # ... the others alternate dense-only, sparse-only by doc id
        dense[f"D{L}"] = np.sort(np.concatenate([docs[both], docs[single[0::2]]]))
        sparse[f"S{L}"] = np.sort(np.concatenate([docs[both], docs[single[1::2]]]))
        assert len(dense[f"D{L}"]) == len(sparse[f"S{L}"]) == L
    # T<n>: the n LOWEST doc ids of DW1 & DW2.  The docs of that intersection tie in [DW1, DW2], so the dense part's top-k is its k lowest
    # ids -- docs of T<n>, there with a partial score: all k of them for n > k, all n of T<n> for n < k
    free = rng.permutation(n)
    inter, rest = np.sort(free[:2210]), free[2210:]
    for t in T_SIZES:
        sparse[f"T{t}"] = inter[:t]
    dense["DW1"] = np.union1d(inter, rest[:800])
    dense["DW2"] = np.union1d(inter, rest[800:1700])
    sparse["U"] = np.union1d(sparse["T1510"][::2], sparse["T1030"][::3])
    core = np.unique(np.concatenate([rng.choice(n, 200, replace=False), sparse["U"][:30], SEAM]))
    sparse["H"] = np.union1d(core, rng.choice(n, 80, replace=False))
    _wide_lists(rng, n, core, dense, [0.22 + 0.025 * i for i in range(11)])
    w = World(n, dl, dense, sparse, 1, 102, exact=True)
    q = w.q
    pairs = sorted(int(x[1:]) for x in sparse if x[0] == "S")
    w.ors += [q([f"S{L}", f"D{L}"]) for L in pairs]
    w.ors += [q([f"S{L}"]) for L in (1, 10, 65, 1025)]
    w.ors += [q(["S10", "S64"]), q(["S129", "S1024"]), q(["S9", "S65", "S257"]), q(["S2", "S11", "S128", "S1023"])]
    w.ors += [q([f"T{t}", "DW1", "DW2"]) for t in T_SIZES]
    # (two pairs: a pair's terms side by side, so that every doc sums its idfs in one order whichever tier holds them)
    w.ors += [q(["S10", "D10", "S64", "D64"]), q(["S129", "D129", "S1024", "D1024"]), q(["S65", "D65", "S256", "D256"]),
              q(["S10", "D10", "S257"]), q(["S64", "D64", "DW1", "DW2"]), q(["S1500", "D1500", "DW2"], nots=["DW1"]),
              q(["S65", "D65"], nots=["DW2", "G3"]),
              # (no dense scored term: the sparse kernel alone answers, and applies the dense NOT terms itself)
              q(["S1025"], nots=["DW1"]), q(["S33", "S64"], nots=["DW2", "G0"]),
              # (a pair beside a long dense list: the dense part is still reading when the sparse part's k-th score arrives as its threshold,
              # and the docs that hold D<L> alone tie with it)
              q(["S10", "D10", "DW1"]), q(["S32", "D32", "DW2"]), q(["S1", "D1", "DW1"]), q(["S33", "D33", "DW1", "DW2"])]
    w.ands += [q([f"S{L}", f"D{L}"], True) for L in (10, 65, 129, 1025, 1500)]
    w.ands += [q([f"T{t}", "DW1", "DW2"], True) for t in (12, 135, 1510)]
    w.ands += [q(["T1030", "DW1"], True), q(["T1510", "U"], True), q(["T1030", "U", "DW2"], True), q(["H", "G0"], True),
               q(["T1510", "DW1"], True, ["D1500"]), q(["T1510", "DW1"], True, ["U"]), q(["T1510", "DW2"], True, ["U", "D1500", "G5"]),
               q(["S1025", "D1025"], True, ["S1024"]), q(["H", "G1", "G2"], True, ["DW1"])]
    w.wide += [q(["H"] + [f"G{i}" for i in range(8)], True), q(["H"] + [f"G{i}" for i in range(11)], True),
               q([f"G{i}" for i in range(4)] + ["H"] + [f"G{i}" for i in range(4, 8)], True, ["DW1"]),
               q(["H"] + [f"G{i}" for i in range(11)], True, ["U"]), q(["H"] + [f"G{i}" for i in range(8)], True, ["U", "DW2"])]
    # unions that exclude a sparse term (bm25_search_tiered_excl): alone, and with a dense NOT term beside it
    w.wide += [q(["DW1"], nots=["T1510"]), q(["S64", "D64"], nots=["U"]), q(["DW1", "DW2"], nots=["T1030", "D1500"]),
               q(["S1025", "D1025"], nots=["S1024"]), q(["S1025", "D1025"], nots=["S1024", "DW2"]), q(["T262", "DW1", "DW2"], nots=["U"])]
    w.deleted = np.unique(np.concatenate([TOMB, w.docs("S1025")[::3]]))
    return w


E_LISTS = {  # dense lists by (sub-block: local docs): segments of 0, 4 (one full 16-byte unit) and 5 (a unit, a posting, padding) postings
    "E1": {0: [0, 17, 100, 4095], 1: [5, 6, 7, 8, 9], 3: [36]},
    "E2": {1: [0, 1, 2, 4095], 2: [0, 2000, 3000, 4000, 4095], 3: [0, 1, 2, 3]},
    "E3": {0: [0, 9, 10, 11, 4095], 2: [1, 2, 3, 4094]},
}


def _build_b(lens=(8, 300)):   # (two lengths under which unequal scores of a query stay clear of the tie band: property (c) below)
    rng = np.random.default_rng(202)
    n = N_DOCS
    cls = rng.integers(0, 6, n)
    dl = np.array([naive.int_to_byte4(x) for x in lens], np.uint8)[cls // 3]
    tf_of = (1 + cls % 3).astype(np.uint16)
    dense, sparse = {}, {}
    for name, segs in E_LISTS.items():
        dense[name] = np.array(sorted(sb * 4096 + x for sb, loc in segs.items() for x in loc))
    dense["DB1"] = np.union1d(SEAM, rng.choice(n, int(0.3 * n), replace=False))
    dense["DB2"] = rng.choice(n, int(0.08 * n), replace=False)
    dense["DB3"] = np.union1d(SEAM, rng.choice(n, int(0.02 * n), replace=False))
    sparse["R1"] = np.array([8192])
    not_seam = np.setdiff1d(np.arange(n), SEAM)
    for L in (63, 64, 65, 511, 512, 513, 1025):
        sparse[f"R{L}"] = np.union1d(SEAM, rng.choice(not_seam, L - len(SEAM), replace=False))
    # the probe list: every sub-block's local docs 0 and 4095, every E segment's first and last posting and the doc behind the last
    probe = {63, 64}
    for sb in range(4):
        probe |= {sb * 4096, min(sb * 4096 + 4095, n - 1)}
        for segs in E_LISTS.values():
            loc = segs.get(sb)
            if loc:
                probe |= {sb * 4096 + loc[0], sb * 4096 + loc[-1]}
                if loc[-1] + 1 < 4096 and sb * 4096 + loc[-1] + 1 < n:
                    probe.add(sb * 4096 + loc[-1] + 1)
    sparse["W"] = np.array(sorted(probe))
    # X ends below 5000, Y -- the next list of the tier's array -- begins with it, Z (shorter than X: it drives) searches X for it
    sparse["X"] = np.sort(rng.choice(np.arange(100, 4990), 200, replace=False))
    sparse["Y"] = np.union1d([5000], rng.choice(np.arange(5001, n), 150, replace=False))
    sparse["Z"] = np.unique(np.concatenate([[5000], sparse["X"][::20], sparse["Y"][5::15], rng.choice(n, 15, replace=False)]))
    sparse["Q"] = np.union1d(sparse["R513"][:470], rng.choice(n, 30, replace=False))   # shares most of its docs with R513
    sparse["V"] = np.sort(rng.choice(n, 300, replace=False))
    core = np.unique(np.concatenate([rng.choice(n, 200, replace=False), sparse["V"][1:90:3], SEAM]))
    sparse["HB"] = np.union1d(core, rng.choice(n, 80, replace=False))
    _wide_lists(rng, n, core, dense, [0.22 + 0.025 * i for i in range(11)])
    # (exact: equal reference scores belong to docs of one weight holding the same terms -- proven below --, which every kernel sums alike)
    w = World(n, dl, dense, sparse, lambda r, d: tf_of[d], 203, exact=True)
    w.cls = cls
    q = w.q
    w.ors += [q([f"R{L}"]) for L in (1, 63, 64, 65, 511, 512, 513, 1025)]
    w.ors += [q(["W", "E1"]), q(["W", "E2"]), q(["W", "E3"]), q(["E1", "W"]), q(["W", "E1", "E2", "E3"]),
              q(["Z", "X"]), q(["X", "Z"]), q(["Z", "X", "Y"]), q(["Y", "Z"]),
              q(["R513", "Q"]), q(["Q", "R513"]), q(["R513", "Q", "DB2"]),
              q(["R65", "DB1"]), q(["R1025", "DB1"]), q(["R513", "DB2", "DB3"]), q(["R512", "R64", "DB3", "DB2"]),
              q(["R1", "R63", "R511", "R1025"]), q(["V", "DB1"]), q(["R1025", "R513", "R65"]), q(["R64", "DB3"]), q(["R63", "DB2"]),
              q(["R511", "DB1", "DB2"]), q(["R65", "DB2"], nots=["DB3"]), q(["R1025", "R64", "DB3"], nots=["DB1", "E2"]),
              q(["R1025", "R513"], nots=["DB1"]), q(["W"], nots=["E1", "E2", "E3"])]
    w.ands += [q(["W", "E1"], True), q(["W", "E2"], True), q(["W", "E3"], True), q(["Z", "X"], True), q(["Z", "X"], True, ["Y"]),
               q(["Z", "DB1"], True, ["X"]), q(["R513", "Q"], True), q(["R513", "Q", "DB1"], True)]
    w.ands += [q([f"R{L}", "DB1"], True) for L in (1, 63, 64, 65, 511, 512, 513, 1025)]
    w.ands += [q(["R513", "DB1", "DB2"], True), q(["V", "DB1"], True, ["DB3"]), q(["R513", "DB1"], True, ["Q"]),
               q(["R1025", "DB1"], True, ["Q", "DB3"]), q(["R1025", "R513"], True), q(["HB", "G0"], True, ["E1"])]
    w.wide += [q(["HB"] + [f"G{i}" for i in range(8)], True), q(["HB"] + [f"G{i}" for i in range(11)], True),
               q([f"G{i}" for i in range(4)] + ["HB"] + [f"G{i}" for i in range(4, 8)], True, ["DB2"]),
               q(["HB"] + [f"G{i}" for i in range(11)], True, ["V"]), q(["HB"] + [f"G{i}" for i in range(8)], True, ["V", "DB2"])]
    w.wide += [q(["DB2"], nots=["R1025"]), q(["R65", "DB1"], nots=["Q"]), q(["W", "E1"], nots=["Z"]), q(["DB1", "DB2"], nots=["R513", "DB3"]),
               q(["R1025"], nots=["R513"]), q(["R513", "Q", "DB3"], nots=["V"]), q(["R512", "DB2"], nots=["R511", "E3"])]
    w.deleted = np.unique(np.concatenate([TOMB, w.docs("V")[::3]]))
    return w


_WORLDS = {}


def _world(name):
    if name not in _WORLDS:
        _WORLDS[name] = {"A": _build_a, "B": _build_b}[name]()
    return _WORLDS[name]


# ---------------------------------------------------------------- the worlds prove themselves (no GPU)
def _sparse_docs(w, terms):
    sp = [w.docs(w.names[t]) for t in terms if w.is_sparse(t)]
    return np.unique(np.concatenate(sp)) if sp else np.zeros(0, np.int64)


def test_world_a_ties_straddle_rank_k_across_the_tiers():
    """(a) for every k some union's exact tie group straddles rank k, holds docs of both tiers, and a dense-only doc of it has a lower
    id than one of its sparse-list docs"""
    w = _world("A")
    for k in KS:
        found = []
        for terms, op_and, nots in w.ors:
            ids, sc, rd, rs = w.c.ref(terms, op_and, nots)
            if len(rd) <= k or rs[k - 1] != rs[k]:
                continue
            group = rd[rs == rs[k - 1]]
            in_sp = np.isin(group, _sparse_docs(w, terms))
            if in_sp.any() and (~in_sp).any() and group[~in_sp].min() < group[in_sp].max():
                found.append(terms)
        print(f"k={k}: {len(found)} unions whose tie group straddles rank k across the tiers, e.g. {[w.names[t] for t in found[0]] if found else None}")
        assert found, k


def test_world_a_dense_docs_at_the_seed():
    """(b) for every k some union has a sparse list of >= k docs (a seed exists: the k-th full score among the sparse lists' docs) and its
    correct top-k holds a dense-only doc scoring exactly that seed"""
    w = _world("A")
    for k in KS:
        found = []
        for terms, op_and, nots in w.ors:
            if not any(not w.is_sparse(t) for t in terms):
                continue
            ids, sc, rd, rs = w.c.ref(terms, op_and, nots)
            sp = _sparse_docs(w, terms)
            sp_sc = np.sort(sc[np.isin(ids, sp)])[::-1]
            if len(sp_sc) < k:
                continue
            seed = sp_sc[k - 1]
            top, top_sc = rd[:k], rs[:k]
            if np.any(~np.isin(top, sp) & (top_sc == seed)):
                found.append(terms)
        print(f"k={k}: {len(found)} unions need dense-only docs scoring exactly the seed, e.g. {[w.names[t] for t in found[0]] if found else None}")
        assert found, k


def test_world_a_sparse_docs_fill_the_dense_top_k():
    """for every k some [T<n>, DW1, DW2] with n > k has a dense part ([DW1, DW2] alone) whose reference top-k is docs of T<n> ONLY -- k
    partial-score entries, every one to be dropped for the sparse list's full-score entry -- and (k > 1) one with k / 2 <= n < k has
    all n docs of T<n> in it, beside the k - n docs without the sparse term that the answer needs from that list"""
    w = _world("A")
    dw = [w.id["DW1"], w.id["DW2"]]
    rd = w.c.ref(dw, False, ())[2]
    for k in KS:
        inside = {t: int(np.isin(rd[:k], w.docs(f"T{t}")).sum()) for t in T_SIZES}
        above = [t for t in T_SIZES if t > k and inside[t] == k]
        below = [t for t in T_SIZES if k / 2 <= t < k and inside[t] == t]
        print(f"k={k}: docs of T<n> in the dense top-k: {inside}")
        assert above and (below or k == 1), (k, inside)
        for t in above + below:
            assert w.q([f"T{t}", "DW1", "DW2"]) in w.ors


@pytest.mark.parametrize("name", ["A", "B"])
def test_scores_are_bit_equal_or_clear_of_the_tie_band(name):
    """(c) outside bit-equal groups any two reference scores of a query differ by more than twice the tie band (REL of the larger): the
    "docs above the tie band" check of _check then leaves out no rank that is not an exact tie of the k-th -- the share left out is 0.
    World B runs with exact_ties as well (more than the bit-equal groups in doc-id order that _check enforces without it: the tie at
    rank k must go to the lowest doc ids): its bit-equal groups are docs of one weight that hold the same terms of the query"""
    w = _world(name)
    ranks = left = 0
    for deleted in ((), w.deleted):
        for terms, op_and, nots in w.all_queries():
            ids, sc, rd, rs = w.c.ref(terms, op_and, nots, deleted)
            u = np.unique(rs)
            if len(u) > 1:
                gap = np.diff(u) / u[1:]
                assert gap.min() > 2 * REL, f"{[w.names[t] for t in terms]} NOT {[w.names[t] for t in nots]}: scores {u[np.argmin(gap)]!r} and " \
                                            f"{u[np.argmin(gap) + 1]!r} are {gap.min():.3g} apart"
            if name == "B":   # a bit-equal group: docs of ONE weight class that hold the same terms of the query
                sig = w.cls[rd] << len(terms)
                for j, t in enumerate(terms):
                    sig |= np.isin(rd, w.docs(w.names[t])).astype(np.int64) << j
                assert np.all((sig[1:] == sig[:-1])[rs[1:] == rs[:-1]]), [w.names[t] for t in terms]
            for k in KS:
                n = min(k, len(rs))
                if n:
                    kth = rs[n - 1]
                    ranks += n
                    left += int(np.sum((rs[:n] > kth) & (rs[:n] <= kth + abs(kth) * REL)))
    print(f"world {name}: {left} of {ranks} ranks inside a tie band without being an exact tie ({left / max(ranks, 1):.2%})")
    assert left == 0


def test_world_b_segments_and_seams():
    """(d) the dense segment shapes (0, 4 and 5 postings) occur and are probed -- a doc behind the last posting, local docs 0 and 4095 --
    by a sparse list; the sparse lists' lengths, the seam docs, X / Y / Z and the two lists sharing their docs are what the docstring says"""
    w = _world("B")
    probe = w.docs("W")
    seen = set()
    for name, segs in E_LISTS.items():
        d = w.docs(name)
        for sb in range(4):
            seg = d[(d >> 12) == sb]
            assert len(seg) == len(segs.get(sb, []))
            seen.add(len(seg))
            lo, hi = sb * 4096, min(sb * 4096 + 4095, N_DOCS - 1)
            assert lo in probe and hi in probe
            if len(seg) and seg[-1] < hi:
                assert seg[-1] + 1 in probe and seg[-1] + 1 not in seg
            if len(seg) in (4, 5):
                assert np.isin(seg, probe).any()   # (and a hit)
    assert {0, 4, 5} <= seen
    assert [len(w.docs(f"R{L}")) for L in (1, 63, 64, 65, 511, 512, 513, 1025)] == [1, 63, 64, 65, 511, 512, 513, 1025]
    for L in (63, 64, 65, 511, 512, 513, 1025):
        assert np.isin(SEAM, w.docs(f"R{L}")).all()
    x, y, z = w.docs("X"), w.docs("Y"), w.docs("Z")
    assert w.id["Y"] == w.id["X"] + 1 and x[-1] < y[0] and y[0] in z and len(z) < len(x)
    assert len(np.intersect1d(w.docs("R513"), w.docs("Q"))) >= 0.9 * len(w.docs("Q"))
    assert np.isin(TOMB, w.deleted).all() and np.isin(w.docs("V")[::3], w.deleted).all()
    print("segment sizes of E1 / E2 / E3 by sub-block:", {n: [len(s.get(sb, [])) for sb in range(4)] for n, s in E_LISTS.items()})


@pytest.mark.parametrize("name", ["A", "B"])
def test_worlds_hold_every_query_kind(name):
    """unions of 1 .. 4 terms in every tier mix, intersections of 2 / 3 terms, of 9 and of 12 with one sparse term, NOT terms of either
    tier in intersections, unions excluding a sparse term alone and with a dense NOT term beside it; the wide intersections match on both
    sides of some k"""
    w = _world(name)
    mixes = {(len(t), sum(w.is_sparse(x) for x in t)) for t, op, nots in w.ors}
    assert {(1, 1), (2, 1), (2, 2), (3, 1), (3, 2), (3, 3), (4, 1), (4, 2), (4, 4)} <= mixes, mixes   # (terms, sparse ones among them)
    assert {len(t) for t, op, nots in w.ands} >= {2, 3} and all(any(w.is_sparse(x) for x in t) for t, op, nots in w.ands + w.wide if op)
    wide = [(t, nots) for t, op, nots in w.wide if op]
    assert {len(t) for t, nots in wide} == {9, 12} and all(sum(w.is_sparse(x) for x in t) == 1 for t, nots in wide)
    for qs in (w.ands, wide):
        assert any(nots and all(not w.is_sparse(x) for x in nots) for *_, nots in qs) and any(any(w.is_sparse(x) for x in nots) for *_, nots in qs)
    excl = [(t, nots) for t, op, nots in w.wide if not op]
    assert all(any(w.is_sparse(x) for x in nots) for t, nots in excl)
    assert any(all(w.is_sparse(x) for x in nots) for t, nots in excl) and any(not all(w.is_sparse(x) for x in nots) for t, nots in excl)
    totals = [len(w.c.ref(t, True, nots)[0]) for t, nots in wide]
    assert min(totals) > 10 and max(totals) > 129, totals


_RT = types.SimpleNamespace(ResultType=types.SimpleNamespace(Topk="topk", TopkCount="topkcount", Count="count"))


def test_the_checks_reject_altered_answers():
    """_check on hand-altered answers of world A's [S10, D10] at k = 10 (three docs hold both terms, the other seven places go to the lowest
    ids of the tie group, dense-only docs among them): a doc twice, a doc of both lists with its dense-only score, the last dense-only doc
    at the seed's score replaced by the next sparse doc -- each must be refused; the unaltered answer passes"""
    w = _world("A")
    terms, op_and, nots = w.q(["S10", "D10"])
    k = 10
    ids, sc, rd, rs = w.c.ref(terms, op_and, nots)
    sp = w.docs("S10")

    def check(d, s):
        d, s = np.asarray(d, np.uint32), np.asarray(s, np.float32)
        _check(w.c, "altered", terms, op_and, nots, (), k, _RT.ResultType.TopkCount, d, s, len(d), len(ids), _RT, exact_ties=True)

    good_d, good_s = rd[:k].copy(), rs[:k].astype(np.float32)
    check(good_d, good_s)
    d = good_d.copy()
    d[5] = d[4]
    with pytest.raises(AssertionError, match="a doc twice"):
        check(d, good_s)
    assert rs[0] > rs[k - 1] and rd[0] in sp           # rank 0 holds both terms; with its dense-only score it falls into the tie group
    rest_d, rest_s = good_d[1:], good_s[1:]
    d, s = np.append(rest_d, good_d[0]), np.append(rest_s, good_s[-1])
    order = np.lexsort((d, -s.astype(np.float64)))
    with pytest.raises(AssertionError, match="scored"):
        check(d[order], s[order])
    tie = np.nonzero(good_s == good_s[-1])[0]
    dense_only = [i for i in tie if good_d[i] not in sp]
    beyond = [x for x, y in zip(rd[k:], rs[k:]) if y == rs[k - 1] and x in sp]
    assert dense_only and beyond
    d = good_d.copy()
    d[dense_only[-1]] = beyond[0]
    order = np.lexsort((d, -good_s.astype(np.float64)))
    with pytest.raises(AssertionError, match="lowest doc ids first"):
        check(d[order], good_s)


# ---------------------------------------------------------------- the GPU
@pytest.fixture(scope="module")
def S():
    import seekstorm_amd
    return seekstorm_amd


@pytest.fixture(scope="module")
def N():
    from seekstorm_amd import _native
    return _native


def _shard(S, w):
    c = w.c
    e = int(c.offs[w.nd])
    sh = S.Shard(0)
    sh.upload_lexical(c.n_docs, c.doclen, c.offs[:w.nd + 1], c.docs[:e], c.tfs[:e])
    # two appends (the ids and the tier's array continue); world B: the second one begins with Y, right behind X
    cut = w.id.get("Y", (w.nd + len(w.names)) // 2)
    m = int(c.offs[cut])
    assert sh.append_sparse(c.offs[w.nd:cut + 1] - c.offs[w.nd], c.docs[e:m], c.tfs[e:m]) == w.nd
    assert sh.append_sparse(c.offs[cut:] - c.offs[cut], c.docs[m:], c.tfs[m:]) == cut
    assert sh.sparse_info()[:2] == (len(w.names) - w.nd, len(c.docs) - e)
    assert [int(x) for x in sh.posting_count(np.arange(len(w.names)))] == [len(d) for d, _ in c.lists]
    return sh


@pytest.fixture(scope="module")
def shard_a(S):
    sh = _shard(S, _world("A"))
    yield sh
    sh.close()


@pytest.fixture(scope="module")
def shard_b(S):
    sh = _shard(S, _world("B"))
    yield sh
    sh.close()


class _Counted:
    """the shard, with the path counters read around every search"""
    def __init__(self, sh, N):
        self._sh, self._strategy, self.calls = sh, N.BM25_AUTO, []

    def __getattr__(self, name):
        return getattr(self._sh, name)

    def set_strategy(self, strategy):
        self._strategy = strategy
        self._sh.set_strategy(strategy)

    def search_lexical_batch(self, q, k, rt, **kw):
        one, gen = self._sh.one_launch_batches(), self._sh.generic_batches()
        out = self._sh.search_lexical_batch(q, k, rt, **kw)
        self.calls.append((self._strategy, len(q), k, rt, self._sh.one_launch_batches() - one, self._sh.generic_batches() - gen))
        return out


def _run(S, N, w, sh, qs, deleted, fits_one_launch):
    """every query of qs (one op at a time, as _run_all batches them): the set as it is at every k under both strategies, then repeated
    beyond the one-launch path's 256 queries at the k it serves -- the staged tiered pipeline with seeds; then the path counters"""
    cs = _Counted(sh, N)
    sh.set_deleted(deleted)
    try:
        _run_all(S, N, cs, w.c, qs, deleted=deleted, strategies=(N.BM25_AUTO, N.BM25_EXHAUSTIVE), ks=KS, exact_ties=w.exact)
        small = len(cs.calls)
        for op_and in (False, True):
            sub = [x for x in qs if x[1] == op_and]
            if sub:
                _run_all(S, N, cs, w.c, sub * (ONE_LAUNCH_MAX_Q // len(sub) + 1), deleted=deleted, strategies=(N.BM25_AUTO,),
                         ks=tuple(k for k in KS if k <= ONE_LAUNCH_MAX_K), exact_ties=w.exact)
    finally:
        sh.set_deleted([])
    seen = {"one launch": 0, "staged, > 256 queries": 0, "staged, k > 32": 0, "staged, exhaustive": 0, "staged, counts only": 0, "staged, shape": 0}
    for i, (strategy, nq, k, rt, one, gen) in enumerate(cs.calls):
        what = (strategy, nq, k, int(rt), one, gen)
        assert gen == 0, what          # (one indexed field, no filter: the sparse kernel drives the wide intersections too)
        takes = strategy == N.BM25_AUTO and rt != S.ResultType.Count and nq <= ONE_LAUNCH_MAX_Q and k <= ONE_LAUNCH_MAX_K and fits_one_launch
        assert one == (1 if takes else 0), what
        key = "one launch" if takes else "staged, > 256 queries" if nq > ONE_LAUNCH_MAX_Q else "staged, exhaustive" if strategy != N.BM25_AUTO \
            else "staged, k > 32" if k > ONE_LAUNCH_MAX_K else "staged, counts only" if rt == S.ResultType.Count else "staged, shape"
        seen[key] += 1
    assert any(nq > ONE_LAUNCH_MAX_Q for _, nq, *_ in cs.calls[small:]) and all(nq <= 64 for _, nq, *_ in cs.calls[:small])
    print("calls by path:", seen)
    return seen


@pytest.mark.gpu
@pytest.mark.parametrize("tombstones", [False, True])
@pytest.mark.parametrize("op", ["or", "and"])
def test_world_a_small_shapes(S, N, shard_a, op, tombstones):
    """determined ties: unions of 1 .. 4 terms in every tier mix / intersections of 2 and 3 terms with a sparse driver, NOT terms -- the
    one-launch path (role 3) for calls of <= 64 queries at k <= 32, the staged pipeline with seeds otherwise; the reference's very list"""
    w = _world("A")
    seen = _run(S, N, w, shard_a, w.ors if op == "or" else w.ands, w.deleted if tombstones else (), True)
    assert seen["one launch"] and seen["staged, > 256 queries"] and seen["staged, k > 32"] and seen["staged, exhaustive"]


@pytest.mark.gpu
@pytest.mark.parametrize("tombstones", [False, True])
def test_world_a_wide_intersections_and_excluding_unions(S, N, shard_a, tombstones):
    """9- and 12-term intersections with one sparse term (the sparse kernel drives them), unions that exclude a sparse term
    (bm25_search_tiered_excl): never the one-launch path"""
    w = _world("A")
    seen = _run(S, N, w, shard_a, w.wide, w.deleted if tombstones else (), False)
    assert not seen["one launch"] and seen["staged, shape"]


@pytest.mark.gpu
@pytest.mark.parametrize("tombstones", [False, True])
@pytest.mark.parametrize("op", ["or", "and"])
def test_world_b_small_shapes(S, N, shard_b, op, tombstones):
    """seams: list lengths on the sparse kernel's steps, postings on word and sub-block seams, sp_find at a list's end, dense_find in
    empty / full-unit / padded segments"""
    w = _world("B")
    seen = _run(S, N, w, shard_b, w.ors if op == "or" else w.ands, w.deleted if tombstones else (), True)
    assert seen["one launch"] and seen["staged, > 256 queries"] and seen["staged, k > 32"] and seen["staged, exhaustive"]


@pytest.mark.gpu
@pytest.mark.parametrize("tombstones", [False, True])
def test_world_b_wide_intersections_and_excluding_unions(S, N, shard_b, tombstones):
    w = _world("B")
    seen = _run(S, N, w, shard_b, w.wide, w.deleted if tombstones else (), False)
    assert not seen["one launch"] and seen["staged, shape"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["A", "B"])
def test_one_call_mixing_every_shape(S, N, shard_a, shard_b, name):
    """every query of a world, shuffled, in ONE call: unions, intersections, the wide ones and the unions that exclude a sparse term side
    by side -- the call is split by shape (one launch for what fits, the staged tiered pipeline, bm25_search_tiered_excl's single
    answers put back into their rows) and every row must come back in the caller's order; once as it is, once repeated beyond 256"""
    w, sh = _world(name), shard_a if name == "A" else shard_b
    qs = w.all_queries()
    qs = [qs[i] for i in np.random.default_rng(7).permutation(len(qs))]
    q = sh.make_queries([x[0] for x in qs], [S.QueryType.Intersection if x[1] else S.QueryType.Union for x in qs], [list(x[2]) for x in qs])
    try:
        for deleted in ((), w.deleted):
            sh.set_deleted(deleted)
            for strategy in (N.BM25_AUTO, N.BM25_EXHAUSTIVE):
                sh.set_strategy(strategy)
                for reps in (1, ONE_LAUNCH_MAX_Q // len(qs) + 1):
                    qq = np.concatenate([q] * reps)
                    for k, rt in ((10, S.ResultType.TopkCount), (10, S.ResultType.Topk), (10, S.ResultType.Count), (32, S.ResultType.TopkCount),
                                  (129, S.ResultType.TopkCount), (1500, S.ResultType.Topk)):
                        one = sh.one_launch_batches()
                        d, s, cnt, tot = sh.search_lexical_batch(qq, k, rt, reference_shortcuts=False)
                        takes = strategy == N.BM25_AUTO and rt != S.ResultType.Count and len(qq) <= ONE_LAUNCH_MAX_Q and k <= ONE_LAUNCH_MAX_K
                        assert sh.one_launch_batches() - one == (1 if takes else 0), (strategy, len(qq), k, int(rt))
                        for j in range(len(qq)):
                            terms, op_and, nots = qs[j % len(qs)]
                            where = f"mixed call of {len(qq)}, row {j}, strategy {strategy} k={k} rt={int(rt)} {'AND' if op_and else 'OR'} " \
                                    f"{[w.names[x] for x in terms]} NOT {[w.names[x] for x in nots]}"
                            _check(w.c, where, terms, op_and, nots, deleted, k, rt, d[j], s[j], cnt[j], tot[j], S, w.exact)
    finally:
        sh.set_strategy(N.BM25_AUTO)
        sh.set_deleted([])


@pytest.mark.gpu
def test_world_a_through_the_device_pointer_entry_point(S, N, shard_a):
    """world A's unions as a device-resident batch that declares sparse terms (ops_mask bit 28): split on the host, always staged"""
    import torch
    w, sh = _world("A"), shard_a
    q = sh.make_queries([x[0] for x in w.ors], S.QueryType.Union, [list(x[2]) for x in w.ors])
    nq = len(q)
    qd = torch.from_numpy(q.view(np.uint8).reshape(nq, -1).copy()).cuda()
    for k in (10, 129):
        doc = torch.full((nq, k), -1, dtype=torch.int32, device="cuda")
        score = torch.zeros((nq, k), dtype=torch.float32, device="cuda")
        cnt = torch.zeros(nq, dtype=torch.int32, device="cuda")
        tot = torch.zeros(nq, dtype=torch.int64, device="cuda")
        one = sh.one_launch_batches()
        N.check(N.lib().ss_bm25_search_dev(sh._h, nq, qd.data_ptr(), k, int(S.ResultType.TopkCount), 1 << 28, doc.data_ptr(), score.data_ptr(),
                                           cnt.data_ptr(), tot.data_ptr(), None), "ss_bm25_search_dev")
        torch.cuda.synchronize()
        assert sh.one_launch_batches() == one
        d, s, c, t = doc.cpu().numpy().view(np.uint32), score.cpu().numpy(), cnt.cpu().numpy().view(np.uint32), tot.cpu().numpy().view(np.uint64)
        for i, (terms, op_and, nots) in enumerate(w.ors):
            _check(w.c, f"device entry k={k} {[w.names[x] for x in terms]}", terms, op_and, nots, (), k, S.ResultType.TopkCount, d[i], s[i], c[i], t[i],
                   S, exact_ties=True)
