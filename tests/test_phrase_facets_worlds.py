"""The corpora of tests/test_gpu_phrase_facets.py, on the oracle alone (no GPU): each one must give the refine kernel something to do --
for at least three phrases 0 < |phrase set| < |intersection set of the same words| -- and must hold the planted edge docs (doc 0, the
last doc, 4095 / 4096, a doc that is the only candidate of its 64-doc group).  The builders assert all of it themselves; a seed or a
size that stops giving it fails here, before any device run."""
import pytest

import test_gpu_phrase_facets as T


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


def test_dense_world_is_not_vacuous(O):
    W = T._dense_world(O)
    assert W.lonely % 64 == 37 and W.lonely not in T.EDGE_DOCS
    sizes = [len(T._matches(W, O, ph, neg, False)[0]) for ph, neg in T.DENSE_CASES]
    assert min(sizes) == 0 and max(sizes) > 1024 and sum(1 for s in sizes if 0 < s < 10_000) >= 10  # an empty set, a deep one, the rest in between


def test_fields_world_is_not_vacuous(O):
    W = T._fields_world(O)
    assert all(len(T._fields_matches(W, O, ph, filt, True)[0]) <= len(T._fields_matches(W, O, ph, filt, False)[0]) for ph, filt in T.F_CASES)


def test_sparse_world_is_not_vacuous(O):
    W = T._sparse_world(O)
    assert all(len(T._matches(W, O, ph, neg, False)[0]) > 0 for ph, neg in T.SP_CASES)
