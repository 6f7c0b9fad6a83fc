"""The worlds of tests/phrase_edge_world.py are what they claim -- shown on the CPU, before any kernel reads them:
  oracle agreement   the definition, the oracle's restated reference loop and the oracle's own definition give the same sets;
  not vacuous        every named doc is a candidate of its phrase and matches (or not) as its case says, the refine has work to do,
                     every match set fits a page of 100, every rich_miss doc outscores every real match of "A B", fill holds no phrase;
  slots              the named docs are the first / last posting of their lists and the first posting behind a padded segment, and
                     each of A, B, C is the shortest list of some phrase."""
import numpy as np
import pytest

import phrase_edge_world as PW


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module", params=[1, 2], ids=["one_field", "three_fields"])
def W(request):
    return PW.world(request.param)


_ORACLE = {}  # world name -> its oracle shard (one field) / its upload arrays (three), built once


def _oracle_sets(O, W, ph, dead):
    """the phrase's match set by the oracle's two forms (NOT lists applied here: the oracle's phrase entry takes none)"""
    terms = W.untiered
    uniq = [terms.index(t) for t in ph.uniq]
    seq = [ph.uniq.index(w) for w in ph.words]
    gone = W.gone if dead else []
    out = []
    for loop in (True, False):
        if W.n_fields == 1:
            if W.name not in _ORACLE:
                offs, docs, tfs, positions = W.csr(terms)
                _ORACLE[W.name] = O.Shard(W.n_docs, W.doclen, offs, docs, tfs)
                _ORACLE[W.name].set_positions(positions)
            _ORACLE[W.name].set_deleted(gone)
            od, _, tot = _ORACLE[W.name].search_phrase(uniq, seq, W.n_docs, reference_loop=loop)
        else:
            if W.name not in _ORACLE:
                _ORACLE[W.name] = W.csr(terms)
            offs, docs, fields, tfs, positions = _ORACLE[W.name]
            od, _, tot = O.search_fields_phrase(W.n_docs, W.doclen, W.boost, offs, docs, fields, tfs, positions, uniq, seq, W.n_docs, deleted=gone,
                                                field_filter=ph.filt, reference_loop=loop)
        assert len(od) == tot
        drop = np.concatenate([W.term_docs(t) for t in ph.nots]) if ph.nots else np.zeros(0, np.int64)
        out.append(np.sort(od.astype(np.int64)[~np.isin(od, drop)]))
    return out


@pytest.mark.parametrize("dead", [False, True], ids=["live", "tombstones"])
def test_the_definition_and_both_oracle_forms_agree(O, W, dead):
    for ph in W.table:
        want = W.matches(ph, dead)
        loop, plain = _oracle_sets(O, W, ph, dead)
        assert np.array_equal(loop, want), (W.name, ph, "reference loop", W.names(np.setxor1d(loop, want)))
        assert np.array_equal(plain, want), (W.name, ph, "oracle definition", W.names(np.setxor1d(plain, want)))


def test_the_cases_are_not_vacuous(W):
    used = {ph.words for ph in W.table}
    for case, doc, words, filt, ok in W.claims:
        assert words in used, (case, words, "no phrase of the table meets this case")
        assert doc in W.intersection(words), (case, doc, words, "not a candidate")
        assert W.doc_matches(doc, words, filt) == ok, (case, doc, words, filt)
    refined = 0
    for ph in W.table:
        m, cand = W.matches(ph), W.intersection(ph.uniq)
        assert 0 < len(m) < 100, (ph, len(m))
        refined += len(m) < len(cand)
        assert set(m.tolist()) <= W.reserved, (ph, "fill forms a phrase", sorted(set(m.tolist()) - W.reserved))
        assert len(W.matches(ph, True)) < len(m) or not set(m.tolist()) & set(W.gone), ph
    assert refined >= 6
    # fill alone is even: no position of a doc outside the reserved ones is odd
    for t, lists in W.pos.items():
        for key, ps in lists.items():
            d = key if W.n_fields == 1 else key[0]
            assert d in W.reserved or all(p % 2 == 0 for p in ps), (t, key)
    ab = PW.Phrase(("A", "B"))
    assert set(W.gone_edges) <= set(W.matches(ab).tolist()) and not set(W.gone_edges) & set(W.matches(ab, True).tolist())
    assert max(len(ps) for lists in W.pos.values() for ps in lists.values()) == (PW.LONG_LIST if W.n_fields == 1 else 1000)


def test_every_rich_miss_doc_outscores_every_real_match():
    W = PW.world(1)
    ab = PW.Phrase(("A", "B"))
    sc = W.scores(ab.uniq)
    docs, scores = W.expected(ab)
    worst_rich = min(sc[d] for d in W.rich)
    assert len(W.rich) == 30 and float(scores[0]) < worst_rich, (float(scores[0]), worst_rich)
    assert all(len(W.pos[t][d]) >= 40 for t in "AB" for d in W.rich) and not set(W.rich) & set(docs.tolist())
    # ... so the best k docs of the intersection are near misses for k = 1 and 10
    top = sorted(sc, key=lambda d: -sc[d])[:30]
    assert set(top) == set(W.rich)


def test_the_named_docs_sit_in_the_slots_they_are_named_for(W):
    for kind, t, doc in W.slots:
        docs = W.term_docs(t).tolist()
        seg = lambda s: [d for d in docs if d // PW.SUB == s]
        if kind == "first_of_list":
            assert docs[0] == doc, (kind, t, doc)
        elif kind == "last_of_list":
            assert docs[-1] == doc, (kind, t, doc)
        else:  # the first posting of its segment; the segment before it ends in NULL padding (segments are padded to 4 postings)
            s = doc // PW.SUB
            assert seg(s)[0] == doc and len(seg(s - 1)) % 4 != 0, (kind, t, doc, len(seg(s - 1)))
            if s == 1:
                assert len(seg(s)) % 4 != 0, (kind, t, doc, len(seg(s)))
    # in the tiered form A's doc 0 is the sparse tier's very first posting
    assert W.sparse[0] == "A" and W.term_docs("A")[0] == 0
    # each of these lists is the shortest of a phrase in use
    used = {ph.words for ph in W.table}
    for t, words in W.drivers.items():
        assert words in used and min(set(words), key=lambda x: len(W.term_docs(x))) == t, (t, words)
    assert {"A", "B", "C"} <= set(W.drivers)
    n = {t: len(W.term_docs(t)) for t in W.pos}
    assert n["A"] < n["B"] < n["C"]
    if W.n_fields == 1:
        assert max(n["D"], n["E"]) < n["A"]
