"""The last stage of every multi-shard and every hybrid search (search.rs:1875-2119) at its edges (-m gpu), held bit for bit to
naive.merge_exact -- ids, f32 scores, sources, counts, the UINT64_MAX padding and the totals:
  a. ss_topk_merge_dev / ss_topk_merge_dev_packed / ss_topk_concat_dev_packed on gathered buffers built on the host: 1 - 16 shards,
     k from 1, n_shards * k at the LDS sort's 8192-key seam (8191 / 8192 / 8193: both kernels, non-power-of-two padding), counts of
     0, below k, above k and UINT32_MAX, scores from the edge palette (exact ties across shards, -0.0 beside +0.0 in the order the
     reference's stable sort leaves them, -inf, subnormals);
  b. ss_rrf_merge_dev: u32 and u64 ids (above 2^32), k_lex + k_vec at 8192 and 8193 (SS_ENOTSUP), absent / empty / UINT32_MAX
     lists, overlapping and disjoint lists, many equal fused scores, offsets inside, at and past the fused length;
  c. hybrid searches end to end on real images -- Index.search over 1 - 3 shards, ss_hybrid_search_sharded on one rank (device and
     host fusion), ss_bm25_search_dev + ss_vec_search_dev -> ss_rrf_merge_dev.  Determined worlds (integer vector dots, lexical
     scores from few (tf, length byte) pairs, the same data in every shard): each leg is the exact one, tie rules included.
     General worlds (f32 Dot / Euclidean, NOT terms, tombstones, a facet filter, Nprobe): each leg meets its exact reference up to
     rounding; the fused page is merge_exact over the legs as returned."""
import numpy as np
import pytest

from oracle import naive

pytestmark = pytest.mark.gpu
U32_MAX, U64_MAX = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF
REL = 1e-4


@pytest.fixture(scope="module")
def S():
    import seekstorm_amd
    return seekstorm_amd


@pytest.fixture(scope="module")
def N():
    from seekstorm_amd import _native
    return _native


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def _assert_page(where, doc, score, cnt, want, src=None):
    """one query's device page [out_len] against merge_exact's (doc, score, source, _)"""
    wd, ws, wsrc = want[0], want[1], want[2]
    n = len(wd)
    assert int(cnt) == n, f"{where}: count {int(cnt)}, want {n}"
    d = np.asarray(doc).view(np.uint64)
    bad = np.nonzero(d[:n] != wd)[0]
    assert len(bad) == 0, f"{where}: position {bad[0]}: doc {int(d[bad[0]])}, want {int(wd[bad[0]])} (score {score[bad[0]]!r}, want {ws[bad[0]]!r})"
    bad = np.nonzero(_bits(score[:n]) != _bits(ws))[0]
    assert len(bad) == 0, f"{where}: position {bad[0]}: score bits {_bits(score[bad[0]]):#x}, want {_bits(ws[bad[0]]):#x}"
    assert np.all(d[n:] == np.uint64(U64_MAX)), f"{where}: padding past the count"
    if src is not None:
        assert np.array_equal(np.asarray(src[:n]), wsrc), f"{where}: sources"


# ------------------------------------------------------------------ a. gathered buffers
COUNT_KINDS = ("zero", "below", "k", "above", "u32max", "any")


def _gathered(rng, Sn, nq, k):
    doc = rng.integers(0, 1 << 32, (Sn, nq, k), dtype=np.uint64).astype(np.uint32)
    score = np.full((Sn, nq, k), 7.0, np.float32)  # slots past a count: better than any live score -- never to be read
    cnt = np.zeros((Sn, nq), np.uint32)
    for s in range(Sn):
        for q in range(nq):
            kind = COUNT_KINDS[(7 * s + q) % len(COUNT_KINDS)]
            c = {"zero": 0, "below": int(rng.integers(0, k)), "k": k, "above": k + 3, "u32max": U32_MAX,
                 "any": int(rng.integers(0, k + 1))}[kind]
            n = 0 if c == U32_MAX else min(c, k)
            score[s, q, :n] = naive.reference_sorted(rng.choice(naive.MERGE_PALETTE, n))
            cnt[s, q] = c
    return doc, score, cnt


def _want_lists(doc, score, cnt, q):
    out = []
    for s in range(doc.shape[0]):
        c = int(cnt[s, q])
        n = 0 if c == U32_MAX else min(c, doc.shape[2])
        out.append(((doc[s, q, :n], score[s, q, :n]), None))
    return out


@pytest.mark.parametrize("Sn,k", [(1, 1), (2, 1), (3, 1), (8, 1), (9, 1), (16, 1), (3, 5), (8, 7), (9, 100), (16, 64), (2, 4096),
                                  (1, 8191), (1, 8192), (1, 8193), (3, 2731), (8, 1024), (16, 512), (9, 910), (9, 911)])
def test_topk_merges_equal_the_exact_merge(S, N, Sn, k):
    """ss_topk_merge_dev, its packed form (out_len = k) and ss_topk_concat_dev_packed (out_len = n_shards * k): the stable sort of the
    cross-shard concatenation, global ids local * S + shard, counts, padding -- bit for bit"""
    import torch
    rng = np.random.default_rng(1000 * Sn + k)
    nq = len(COUNT_KINDS)
    doc, score, cnt = _gathered(rng, Sn, nq, k)
    dev = torch.device("cuda", 0)
    g_doc = torch.from_numpy(doc.view(np.int32)).to(dev)
    g_score = torch.from_numpy(score).to(dev)
    g_cnt = torch.from_numpy(cnt.view(np.int32)).to(dev)
    packed = np.concatenate([np.concatenate([doc[s].ravel(), score[s].ravel().view(np.uint32), cnt[s]]) for s in range(Sn)])
    g_packed = torch.from_numpy(packed.view(np.int32)).to(dev)
    for name, out_len in (("ss_topk_merge_dev", k), ("ss_topk_merge_dev_packed", k), ("ss_topk_concat_dev_packed", Sn * k)):
        od = torch.full((nq, out_len), 0x5A5A5A5A, dtype=torch.int64, device=dev)
        os_ = torch.full((nq, out_len), 3.0, dtype=torch.float32, device=dev)
        oc = torch.full((nq,), -7, dtype=torch.int32, device=dev)
        f = getattr(N.lib(), name)
        if name == "ss_topk_merge_dev":
            rc = f(0, nq, Sn, k, g_doc.data_ptr(), g_score.data_ptr(), g_cnt.data_ptr(), od.data_ptr(), os_.data_ptr(), oc.data_ptr(), None)
        else:
            rc = f(0, nq, Sn, k, g_packed.data_ptr(), od.data_ptr(), os_.data_ptr(), oc.data_ptr(), None)
        N.check(rc, name)
        torch.cuda.synchronize()
        d, s_, c = od.cpu().numpy().view(np.uint64), os_.cpu().numpy(), oc.cpu().numpy().view(np.uint32)
        for q in range(nq):
            want = naive.merge_exact(naive.MODE_LEXICAL, _want_lists(doc, score, cnt, q), Sn, 0, out_len)
            _assert_page(f"{name} S={Sn} k={k} query {q}", d[q], s_[q], c[q], want)
            assert np.all(_bits(s_[q, len(want[0]):]) == 0), f"{name}: padding scores"


def test_topk_merge_ties_the_two_zeros_in_shard_order(S, N):
    """the hand-worked case: shard 0 holds -0.0, shard 1 +0.0 -- they tie, shard 0 first, each with its own bits; one list
    [1, -0.0, +0.0] beside [+0.0, -0.0] through the rank merge (n_shards * k > 8192) as through the LDS sort"""
    import torch
    dev = torch.device("cuda", 0)
    for k in (5, 5000):  # (out_len = k: all five entries come out)
        Sn, nq = 2, 1
        doc = np.zeros((Sn, nq, k), np.uint32)
        score = np.full((Sn, nq, k), -np.inf, np.float32)
        doc[0, 0, :3], score[0, 0, :3] = [11, 12, 13], [1.0, -0.0, 0.0]
        doc[1, 0, :2], score[1, 0, :2] = [21, 22], [0.0, -0.0]
        cnt = np.array([[3], [2]], np.uint32)
        t = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (doc.view(np.int32), score, cnt.view(np.int32))]
        od = torch.empty((nq, k), dtype=torch.int64, device=dev)
        os_ = torch.empty((nq, k), dtype=torch.float32, device=dev)
        oc = torch.empty((nq,), dtype=torch.int32, device=dev)
        N.check(N.lib().ss_topk_merge_dev(0, nq, Sn, k, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), od.data_ptr(), os_.data_ptr(),
                                          oc.data_ptr(), None), "ss_topk_merge_dev")
        torch.cuda.synchronize()
        n = int(oc[0])
        assert n == 5, (k, n)
        assert od[0, :n].cpu().numpy().tolist() == [22, 24, 26, 43, 45], k
        assert _bits(os_[0, :n].cpu().numpy()).tolist() == _bits([1.0, -0.0, 0.0, 0.0, -0.0]).tolist(), k


# ------------------------------------------------------------------ b. ss_rrf_merge_dev
def _rrf_want(ids, cnt, q, k):
    if ids is None:
        return None
    c = int(cnt[q])
    n = 0 if c == U32_MAX else min(c, k)
    return (ids[q, :n], np.arange(n, 0, -1).astype(np.float32))  # any strictly falling scores: only the ranks enter


def _rrf_run(S, N, lex, vec, offset, length, where):
    """lex / vec: (ids [nq][k] int64 or uint32, counts [nq] uint32) or None -> compare every query with merge_exact"""
    import ctypes as C
    import torch
    dev = torch.device("cuda", 0)
    t = []
    for x in (lex, vec):
        if x is None:
            t.append((None, None))
            continue
        ids, c = x
        ids_t = torch.from_numpy(ids.view(np.int64) if ids.dtype == np.uint64 else ids.view(np.int32)).to(dev)
        t.append((ids_t, torch.from_numpy(c.view(np.int32)).to(dev)))
    st = torch.cuda.current_stream(dev)
    od, os_, src, cnt = S.rrf_merge_device(t[0][0], t[0][1], t[1][0], t[1][1], offset, length, C.c_void_p(st.cuda_stream))
    torch.cuda.synchronize()
    od, os_, src, cnt = od.cpu().numpy().view(np.uint64), os_.cpu().numpy(), src.cpu().numpy(), cnt.cpu().numpy()
    nq = len(od)
    for q in range(nq):
        lists = [(None if lex is None else _rrf_want(lex[0], lex[1], q, lex[0].shape[1]),
                  None if vec is None else _rrf_want(vec[0], vec[1], q, vec[0].shape[1]))]
        want = naive.merge_exact(naive.MODE_HYBRID, lists, 1, offset, length)
        _assert_page(f"{where} offset {offset} length {length} query {q}", od[q], os_[q], cnt[q], want, src[q])
    return cnt


def _ids(rng, n, wide):
    if wide:
        return rng.choice(1 << 20, n, replace=False).astype(np.uint64) * np.uint64(1 << 20) + np.uint64((1 << 33) + 5)  # above 2^32
    return rng.choice(U32_MAX, n, replace=False).astype(np.uint32)  # up to UINT32_MAX - 1


@pytest.mark.parametrize("wide", [False, True], ids=["u32", "u64"])
def test_rrf_merge_equals_the_exact_fusion(S, N, wide):
    rng = np.random.default_rng(77 + wide)
    kl = kv = 100
    nq = 8
    dt = np.uint64 if wide else np.uint32
    ld, vd = np.zeros((nq, kl), dt), np.zeros((nq, kv), dt)
    lc = np.array([kl, kl, kl, 60, kl + 9, 0, kl, 37], np.uint32)
    vc = np.array([kv, kv, kv, 80, kv, kv, U32_MAX, 0], np.uint32)
    for q in range(nq):
        pool = _ids(rng, kl + kv, wide)
        if q == 0:  # fully overlapping lists in random orders
            ld[q], vd[q] = rng.permutation(pool[:kl]), rng.permutation(pool[:kl])
        elif q == 1:  # disjoint lists of one length: every lexical-only rank ties the vector-only rank -> doc ascending
            ld[q], vd[q] = pool[:kl], pool[kl:]
        elif q == 2:  # the vector list is the lexical one reversed: doc (a, b) ties doc (b, a)
            ld[q] = pool[:kl]
            vd[q] = pool[:kl][::-1]
        else:  # partial overlap
            ld[q] = pool[:kl]
            vd[q] = np.concatenate([rng.permutation(pool[:kl])[:kv // 2], pool[kl:kl + kv // 2]])[rng.permutation(kv)]
    where = "u64" if wide else "u32"
    for offset, length in ((0, 10), (0, 200), (7, 30), (99, 2), (150, 60), (199, 5), (200, 10), (260, 4)):
        _rrf_run(S, N, (ld, lc), (vd, vc), offset, length, where)
    # one list absent altogether, one list empty
    _rrf_run(S, N, None, (vd, vc), 3, 120, where + " no lexical list")
    _rrf_run(S, N, (ld, lc), None, 0, 120, where + " no vector list")
    zero = np.zeros(nq, np.uint32)
    _rrf_run(S, N, (ld, zero), (vd, vc), 0, 120, where + " empty lexical list")
    _rrf_run(S, N, (ld, lc), (vd, np.full(nq, U32_MAX, np.uint32)), 0, 120, where + " overflowed vector batch")


def test_rrf_merge_at_its_lds_limit(S, N):
    """k_lex + k_vec = 8192 is answered (two equal halves; 8191 + 1), 8193 is SS_ENOTSUP; many equal fused scores at that size"""
    rng = np.random.default_rng(5)
    nq = 3
    for kl, kv in ((4096, 4096), (8191, 1)):
        pools = [_ids(rng, kl + kv, True) for _ in range(nq)]  # unique ids in each list, as the merge requires
        ld = np.stack([p[:kl] for p in pools])
        vd = np.stack([np.concatenate([rng.permutation(p[:kl])[:kv // 2], p[kl:kl + kv - kv // 2]]) for p in pools])
        lc = np.array([kl, kl // 3, kl], np.uint32)
        vc = np.array([kv, kv, 0], np.uint32)
        for offset, length in ((0, 300), (4000, 500), (kl + kv - 1, 3), (kl + kv, 1)):
            _rrf_run(S, N, (ld, lc), (vd, vc), offset, length, f"k_lex {kl} k_vec {kv}")
    ld = np.stack([_ids(rng, 4097, False) for _ in range(nq)])
    vd = np.stack([_ids(rng, 4096, False) for _ in range(nq)])
    c = np.full(nq, 10, np.uint32)
    with pytest.raises(N.SeekStormHipError) as e:
        _rrf_run(S, N, (ld, c), (vd, c), 0, 10, "8193")
    assert e.value.code == N.SS_ENOTSUP


# ------------------------------------------------------------------ c. hybrid searches end to end
N_DOCS, N_ROWS, DIM = 3000, 700, 32
TERM_DF = (0.05, 0.4, 0.2, 0.1, 0.3)
QUERIES = ([0], [1, 2, 3], [0, 3], [1, 4])


def _lex_world(rng, n_docs, determined):
    """determined: tf in {1, 2}, length byte in {20, 40} -- every doc of one (terms, tfs, lengths) pattern scores the same"""
    if determined:
        doclen = rng.choice(np.array([20, 40], np.uint8), n_docs)
    else:
        doclen = rng.integers(8, 120, n_docs).astype(np.uint8)
    lists = []
    for df in TERM_DF:
        d = np.sort(rng.choice(n_docs, int(df * n_docs), replace=False)).astype(np.uint32)
        tf = rng.integers(1, 3, len(d)) if determined else np.minimum(rng.geometric(0.4, len(d)), 50)
        lists.append((d, tf.astype(np.uint16)))
    return doclen, lists


def _upload_lex(sh, n_docs, doclen, lists):
    offs = np.zeros(len(lists) + 1, np.uint64)
    offs[1:] = np.cumsum([len(d) for d, _ in lists])
    sh.upload_lexical(n_docs, doclen, offs, np.concatenate([d for d, _ in lists]), np.concatenate([t for _, t in lists]))


def _lex_exact(n_docs, doclen, lists, terms, nots=(), deleted=()):
    ids, sc = naive.bm25_exact(n_docs, doclen, [lists[t] for t in terms], False, not_docs=[lists[t][0] for t in nots],
                               deleted=np.asarray(sorted(deleted), np.int64))
    o = np.lexsort((ids, -sc))
    return ids[o].astype(np.int64), sc[o]


def _check_lex_leg(where, d, s, cnt, tot, exact, k, determined):
    ids, sc = exact
    n = min(k, len(ids))
    assert int(cnt) == n and int(tot) == len(ids), f"{where}: count {int(cnt)} / total {int(tot)}, want {n} / {len(ids)}"
    if n == 0:
        return
    d, s = np.asarray(d[:n], np.int64), np.asarray(s[:n], np.float32)
    if determined:  # every leg entry is the exact one: equal scores doc ascending, and bit-equal on the device
        assert np.array_equal(d, ids[:n]), f"{where}: the leg is not the exact order"
        assert np.all(np.abs(s - sc[:n]) <= REL * np.abs(sc[:n])), f"{where}: scores"
        eq = sc[1:n] == sc[:n - 1]
        assert np.all(s[1:][eq] == s[:-1][eq]), f"{where}: exactly equal scores differ on the device"
        return
    pos = {int(x): i for i, x in enumerate(ids)}
    assert len(set(d.tolist())) == n and all(int(x) in pos for x in d), f"{where}: a doc twice or one that does not match"
    own = sc[[pos[int(x)] for x in d]]
    assert np.all(np.abs(s - own) <= REL * np.abs(own)), f"{where}: scores"
    assert np.all(s[1:] <= s[:-1]), f"{where}: scores out of order"
    kth = sc[n - 1]
    band = abs(kth) * REL
    assert set(d[own > kth + band].tolist()) == set(ids[:n][sc[:n] > kth + band].tolist()), f"{where}: docs above the tie band"


def _vec_exact_int(rows, q):
    return (np.asarray(rows, np.int64) @ np.asarray(q, np.int64)).astype(np.float64)


def _check_vec_leg_int(where, d, s, cnt, tot, dots, k):
    """integer dots: the leg is exactly (dot desc, doc asc), scores the dots themselves"""
    o = np.lexsort((np.arange(len(dots)), -dots))
    n = min(k, len(dots))
    assert int(cnt) == n, f"{where}: count {int(cnt)}, want {n}"
    assert np.array_equal(np.asarray(d[:n], np.int64), o[:n]), f"{where}: the leg is not the exact order"
    assert np.array_equal(np.asarray(s[:n], np.float32), dots[o[:n]].astype(np.float32)), f"{where}: scores"
    if len(dots) <= k:
        assert int(tot) == len(dots), f"{where}: total {int(tot)}"


def _int_rows(rng, n, dim):
    return rng.integers(-1, 2, (n, dim)).astype(np.int8)


def _ro_page(ro):
    return (np.array([r.doc_id for r in ro.results], np.uint64), np.array([r.score for r in ro.results], np.float32),
            np.array([int(r.source) for r in ro.results], np.uint8))


def _leg(ro, with_total=True):
    d = np.array([r.doc_id for r in ro.results], np.int64)
    s = np.array([r.score for r in ro.results], np.float32)
    return (d, s, ro.result_count_total) if with_total else (d, s)


def _cmp_ro(where, ro, want):
    d, s, src = _ro_page(ro)
    assert ro.result_count == len(want[0]) == len(d), f"{where}: count {ro.result_count}, want {len(want[0])}"
    assert np.array_equal(d, want[0]), f"{where}: docs {d[:8].tolist()} ..., want {want[0][:8].tolist()} ..."
    assert np.array_equal(_bits(s), _bits(want[1])), f"{where}: fused scores"
    assert np.array_equal(src, want[2]), f"{where}: sources"
    assert ro.result_count_total == want[3], f"{where}: total {ro.result_count_total}, want {want[3]}"


@pytest.mark.parametrize("Sn", [1, 2, 3])
def test_index_hybrid_determined_world(S, Sn):
    """Index.search(Hybrid) over Sn shards that hold the same lexical data and the same i8 rows: every leg is fixed by the tie rules,
    every entry ties its twins in the other shards -- the fused page is merge_exact over the exact legs"""
    rng = np.random.default_rng(300 + Sn)
    doclen, lists = _lex_world(rng, N_DOCS, True)
    rows = _int_rows(rng, N_ROWS, DIM)
    q8 = rng.integers(-1, 2, DIM).astype(np.int8)
    qv = q8.astype(np.float32) / np.float32(127.0)
    assert np.array_equal(S.quantize_f32_to_i8(qv[None])[0], q8)
    dots = _vec_exact_int(rows, q8)
    shards = []
    for sid in range(Sn):
        sh = S.Shard(0, shard_id=sid)
        _upload_lex(sh, N_DOCS, doclen, lists)
        sh.upload_vectors_i8(rows)
        shards.append(sh)
    idx = S.Index(shards)
    try:
        for terms in QUERIES:
            exact = _lex_exact(N_DOCS, doclen, lists, terms)
            for offset, length in ((0, 10), (5, 40), (600, 200), (700, 900), (3000, 5)):
                k = offset + length
                legs = []
                for sid, sh in enumerate(shards):
                    lr = sh.search_lexical_shard(terms, S.QueryType.Union, 0, k, strict=True)
                    vr = sh.search_vector_shard(qv, k, strict=True)
                    ll, vl = _leg(lr), _leg(vr)
                    where = f"S={Sn} shard {sid} terms {terms} k {k}"
                    _check_lex_leg(where + " lexical", ll[0], ll[1], lr.result_count, ll[2], exact, k, True)
                    _check_vec_leg_int(where + " vector", vl[0], vl[1], vr.result_count, vl[2], dots, k)
                    if sid:
                        assert np.array_equal(_bits(ll[1]), _bits(legs[0][0][1])), where + ": twin shards score differently"
                    legs.append((ll, vl))
                want = naive.merge_exact(naive.MODE_HYBRID, legs, Sn, offset, length)
                ro = idx.search(terms, qv, S.QueryType.Union, S.SearchMode.Hybrid, offset, length, strict=True, normalize_query=False)
                _cmp_ro(f"Index S={Sn} terms {terms} offset {offset} length {length}", ro, want)
    finally:
        for sh in shards:
            sh.close()


@pytest.fixture(scope="module")
def f32_int_world(S):
    """one shard: the determined lexical world + f32 rows of integer components (every dot exact in any summation order)"""
    rng = np.random.default_rng(17)
    doclen, lists = _lex_world(rng, N_DOCS, True)
    rows = _int_rows(rng, N_ROWS, DIM).astype(np.float32)
    qs = rng.integers(-1, 2, (len(QUERIES), DIM)).astype(np.float32)
    sh = S.Shard(0)
    _upload_lex(sh, N_DOCS, doclen, lists)
    sh.upload_vectors(rows)
    yield sh, doclen, lists, rows, qs
    sh.close()


def test_hybrid_sharded_single_rank_determined_world(S, f32_int_world):
    """ss_hybrid_search_sharded on one rank at k = offset + length = 1024 (fusion on the device) and 1025 (on the host), offsets past
    0, pages past the fused list: == merge_exact over the shard's exact legs; totals max(lexical, vector)"""
    from seekstorm_amd import distributed as D
    sh, doclen, lists, rows, qs = f32_int_world
    comm = D.ShardComm(0, 1, 0)
    q = sh.make_queries([list(t) for t in QUERIES], S.QueryType.Union)
    try:
        for offset, length in ((1, 1023), (1000, 24), (1, 1024), (1020, 5), (0, 1025)):
            k = offset + length
            hd, hs, hsrc, hc, ht = comm.search_hybrid_sharded(sh, q, qs, offset, length)
            ld, ls, lc, lt = sh.search_lexical_batch(q, k)
            vd, vs, vc, vt = sh.search_vector_batch(qs, k)
            for i, terms in enumerate(QUERIES):
                where = f"sharded terms {terms} offset {offset} length {length}"
                _check_lex_leg(where + " lexical", ld[i], ls[i], lc[i], lt[i], _lex_exact(N_DOCS, doclen, lists, terms), k, True)
                _check_vec_leg_int(where + " vector", vd[i], vs[i], vc[i], vt[i], _vec_exact_int(rows, qs[i]), k)
                legs = [((ld[i, :lc[i]], ls[i, :lc[i]], int(lt[i])), (vd[i, :vc[i]], vs[i, :vc[i]], int(vt[i])))]
                want = naive.merge_exact(naive.MODE_HYBRID, legs, 1, offset, length)
                _assert_page(where, hd[i], hs[i], hc[i], want, hsrc[i])
                assert int(ht[i]) == want[3] == max(int(lt[i]), N_ROWS), where + ": total"
            assert int(hc.min()) < length <= int(hc.max()) or length < 10, "a page past the fused list and a full one"
    finally:
        comm.close()


def test_batched_device_legs_into_rrf_determined_world(S, N, f32_int_world):
    """ss_bm25_search_dev + ss_vec_search_dev -> ss_rrf_merge_dev, never leaving the device: == merge_exact over the exact legs"""
    import ctypes as C
    import torch
    sh, doclen, lists, rows, qs = f32_int_world
    dev = torch.device("cuda", 0)
    q = sh.make_queries([list(t) for t in QUERIES], S.QueryType.Union)
    nq, k = len(q), 300
    st = torch.cuda.Stream(device=dev)
    qd = torch.from_numpy(q.view(np.uint8).reshape(nq, -1).copy()).to(dev)
    tq = torch.from_numpy(qs).to(dev)
    ldoc = torch.full((nq, k), -1, dtype=torch.int32, device=dev); lsc = torch.zeros((nq, k), dtype=torch.float32, device=dev)
    lcnt = torch.zeros((nq,), dtype=torch.int32, device=dev); ltot = torch.zeros((nq,), dtype=torch.int64, device=dev)
    vdoc = torch.full((nq, k), -1, dtype=torch.int32, device=dev); vsc = torch.zeros((nq, k), dtype=torch.float32, device=dev)
    vcnt = torch.zeros((nq,), dtype=torch.int32, device=dev); vtot = torch.zeros((nq,), dtype=torch.int64, device=dev)
    ops = 2 | (3 << 8) | (3 << 16) | (1 << 28)  # unions, <= 3 terms
    N.check(N.lib().ss_bm25_search_dev(sh._h, nq, qd.data_ptr(), k, int(S.ResultType.TopkCount), ops, ldoc.data_ptr(), lsc.data_ptr(),
                                       lcnt.data_ptr(), ltot.data_ptr(), st.cuda_stream), "ss_bm25_search_dev")
    N.check(N.lib().ss_vec_search_dev(sh._h, nq, tq.data_ptr(), k, N.FLT_MIN_NEG, vdoc.data_ptr(), vsc.data_ptr(), vcnt.data_ptr(),
                                      vtot.data_ptr(), st.cuda_stream), "ss_vec_search_dev")
    st.synchronize()
    ld, ls, lc, lt = ldoc.cpu().numpy().view(np.uint32), lsc.cpu().numpy(), lcnt.cpu().numpy().view(np.uint32), ltot.cpu().numpy()
    vd, vs, vc = vdoc.cpu().numpy().view(np.uint32), vsc.cpu().numpy(), vcnt.cpu().numpy().view(np.uint32)
    for i, terms in enumerate(QUERIES):
        _check_lex_leg(f"dev terms {terms} lexical", ld[i], ls[i], lc[i], lt[i], _lex_exact(N_DOCS, doclen, lists, terms), k, True)
        _check_vec_leg_int(f"dev terms {terms} vector", vd[i], vs[i], vc[i], 0, _vec_exact_int(rows, qs[i]), k)
    for offset, length in ((0, 50), (250, 100), (590, 30), (650, 5)):
        with torch.cuda.stream(st):
            od, os_, src, cnt = S.rrf_merge_device(ldoc, lcnt, vdoc, vcnt, offset, length, C.c_void_p(st.cuda_stream))
        st.synchronize()
        od, os_, src, cnt = od.cpu().numpy().view(np.uint64), os_.cpu().numpy(), src.cpu().numpy(), cnt.cpu().numpy()
        for i, terms in enumerate(QUERIES):
            legs = [((ld[i, :lc[i]], ls[i, :lc[i]]), (vd[i, :vc[i]], vs[i, :vc[i]]))]
            want = naive.merge_exact(naive.MODE_HYBRID, legs, 1, offset, length)
            _assert_page(f"dev rrf terms {terms} offset {offset} length {length}", od[i], os_[i], cnt[i], want, src[i])


def _selected_rows(rows, q, lc, child, n_probe, euclid):
    """rows of the clusters AnnMode::Nprobe visits: per level, the n_probe clusters whose medoid (first record) scores best"""
    live = np.zeros(len(rows), bool)
    r0, ci = 0, 0
    for nc in lc:
        starts, r = [], r0
        for j in range(nc):
            starts.append(r)
            r += child[ci + j]
        med = rows[starts]
        sc = -naive.vec_exact_l2(med, q) if euclid else naive.vec_exact_dot(med, q)
        for j in sorted(range(nc), key=lambda j: (-sc[j], j))[:n_probe]:
            live[starts[j]:starts[j] + child[ci + j]] = True
        r0, ci = r, ci + nc
    return live


@pytest.mark.parametrize("Sn", [2, 3])
@pytest.mark.parametrize("sim", ["dot", "euclidean"])
def test_index_hybrid_general_world(S, Sn, sim):
    """f32 Dot / Euclidean rows, NOT terms, tombstones, a facet filter on the lexical leg and Nprobe on the vector leg, a different
    part of the corpus in every shard: each leg meets its exact reference up to rounding (check_vector_topk; bm25_exact), the fused page
    is merge_exact over the legs as returned, the total max(lexical, vector) summed over the shards"""
    euclid = sim == "euclidean"
    rng = np.random.default_rng(500 + Sn + 10 * euclid)
    dim, lc = 48, [3, 2]
    shards, worlds = [], []
    for sid in range(Sn):
        doclen, lists = _lex_world(rng, N_DOCS, False)
        rows = (rng.standard_normal((N_DOCS, dim)) + (2.0 if euclid else 0.0)).astype(np.float32)
        child = [700, 500, 800, 600, 400]
        year = rng.integers(0, 50, N_DOCS).astype("<i2")
        gone = sorted(set(rng.choice(N_DOCS, 60, replace=False).tolist()))
        sh = S.Shard(0, shard_id=sid)
        _upload_lex(sh, N_DOCS, doclen, lists)
        if euclid:
            sh.set_vector_similarity("euclidean")
        sh.upload_vectors(rows)
        sh.set_clusters(lc, child)
        sh.upload_facets(year.view(np.uint8).reshape(N_DOCS, 2))
        sh.set_deleted(gone)
        shards.append(sh)
        worlds.append((doclen, lists, rows, child, year, gone))
    idx = S.Index(shards)
    qv = (rng.standard_normal(dim) + (2.0 if euclid else 0.0)).astype(np.float32)
    ff = [(0, "i16", 10, 40)]
    try:
        for terms, nots in (([1, 2], [3]), ([0, 4], [2]), ([1], [])):
            for offset, length in ((0, 10), (20, 60), (1000, 30)):
                k = offset + length
                legs = []
                for sid, sh in enumerate(shards):
                    doclen, lists, rows, child, year, gone = worlds[sid]
                    where = f"{sim} S={Sn} shard {sid} terms {terms} not {nots} k {k}"
                    lr = sh.search_lexical_shard(terms, S.QueryType.Union, 0, k, strict=True, not_terms=nots, facet_filter=ff)
                    ll = _leg(lr)
                    filtered = set(np.nonzero(~((year >= 10) & (year < 40)))[0].tolist()) | set(gone)
                    _check_lex_leg(where + " lexical", ll[0], ll[1], lr.result_count, ll[2],
                                   _lex_exact(N_DOCS, doclen, lists, terms, nots, filtered), k, False)
                    vr = sh.search_vector_shard(qv, k, strict=True, ann_mode=S.AnnMode.Nprobe(1))
                    vl = _leg(vr)
                    live = _selected_rows(rows, qv, lc, child, 1, euclid)
                    live[gone] = False
                    if euclid:
                        d2 = naive.vec_exact_l2(rows, qv)
                        ex, bd = np.where(live, -d2, -np.inf), naive.bound_l2(rows, qv, d2)
                    else:
                        ex, bd = np.where(live, naive.vec_exact_dot(rows, qv), -np.inf), naive.bound_dot(rows, qv)
                    naive.check_vector_topk(vl[0], vl[1], vr.result_count, ex, bd, k)
                    legs.append((ll, vl))
                want = naive.merge_exact(naive.MODE_HYBRID, legs, Sn, offset, length)
                ro = idx.search(terms, qv, S.QueryType.Union, S.SearchMode.Hybrid, offset, length, strict=True, not_terms=nots,
                                facet_filter=ff, ann_mode=S.AnnMode.Nprobe(1), normalize_query=False)
                _cmp_ro(f"Index {sim} S={Sn} terms {terms} offset {offset} length {length}", ro, want)
    finally:
        for sh in shards:
            sh.close()
