"""Vector scans at their edges (-m gpu) against the exact reference of oracle/naive.py: dims that end a 32-float K chunk one short or
one over, row counts at the 128-row tile seam and the 2048-row first chunk, batches at the 32 / 64-query seams, k up to SS_MAX_K through
every chunk seam, values that cancel or span a wide range, i8 extremes and f32 Euclidean data far from the origin.  Every f32 answer is
held to check_vector_topk: the exact top k up to the rounding band of an f32 sum (bound_dot; bound_l2 for the reference's Euclidean
order); i8 answers are integers and are compared with the C oracle by ==."""
import numpy as np
import pytest

from oracle import naive

pytestmark = pytest.mark.gpu
MAX_K = 1024  # SS_MAX_K


@pytest.fixture(scope="module")
def S():
    import seekstorm_amd
    return seekstorm_amd


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


def _shard(S, rows, euclid, row_doc=None, shard_id=0):
    sh = S.Shard(0, shard_id=shard_id)
    if euclid:
        sh.set_vector_similarity("euclidean")
    sh.upload_vectors(rows, row_doc)
    return sh


def _exact(rows, q, euclid, live=None):
    """(exact similarity, band) of every row; rows outside `live` get -inf"""
    if euclid:
        d2 = naive.vec_exact_l2(rows, q)
        ex, bd = -d2, naive.bound_l2(rows, q, d2)
    else:
        ex, bd = naive.vec_exact_dot(rows, q), naive.bound_dot(rows, q)
    if live is not None:
        ex = np.where(live, ex, -np.inf)
    return ex, bd


def _check(doc, score, cnt, rows, qs, k, euclid, row_doc=None, live=None, O=None, ctx=""):
    for i in range(len(qs)):
        ex, bd = _exact(rows, qs[i], euclid, None if live is None else live[i] if live.ndim == 2 else live)
        try:
            naive.check_vector_topk(doc[i], score[i], cnt[i], ex, bd, k, row_doc=row_doc)
        except AssertionError as e:
            raise AssertionError("%s query %d: %s" % (ctx, i, e)) from None
        if euclid and O is not None:  # the scores stay the reference's own, bit for bit
            n = int(cnt[i])
            if row_doc is None:
                want = [-O.euclidean_f32(qs[i], rows[r], simd_order=rows.shape[1] % 8 == 0) for r in doc[i][:n]]
                assert np.array_equal(score[i][:n], np.float32(want)), (ctx, i)


def _gen(seed, n, dim, scale=1.0):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, dim)) * scale).astype(np.float32)


# ---------------------------------------------------------------- shapes
DIMS = [1, 2, 7, 8, 9, 31, 33, 63, 65, 127, 129, 255, 257, 1000, 1536]


@pytest.mark.parametrize("dim", DIMS + [30, 62, 94])
def test_dims(S, O, dim):
    """2049 rows (one past the 16-tile first chunk), 3 queries, k = 1, 10 and SS_MAX_K; Dot on centred data, Euclidean off the
    origin (dims 30, 62, 94: dim + 2 augmented columns land on / one past a 32-column boundary)"""
    n = 2049
    for euclid in ((False, True) if dim in DIMS else (True,)):
        rows = naive.vec_offcentre(dim, n, dim, 30.0, 0.05) if euclid else _gen(dim, n, dim)
        qs = naive.vec_offcentre(dim + 1, 3, dim, 30.0, 0.05) if euclid else _gen(dim + 1, 3, dim)
        sh = _shard(S, rows, euclid)
        for k in (1, 10, MAX_K):
            doc, score, cnt, _ = sh.search_vector_batch(qs, k)
            _check(doc, score, cnt, rows, qs, k, euclid, O=O, ctx="dim %d euclid %s k %d" % (dim, euclid, k))
        sh.close()


@pytest.mark.parametrize("euclid", [False, True])
def test_row_counts(S, O, euclid):
    """tile seams (127 / 128 / 129), k - 1 / k / k + 1 rows, the first chunk's seam (2047 / 2048 / 2049) and an image of several
    growth chunks"""
    dim, k = 40, 100
    big = naive.vec_offcentre(7, 60_000, dim, 100.0, 0.3) if euclid else _gen(7, 60_000, dim)
    qs = naive.vec_offcentre(8, 4, dim, 100.0, 0.3) if euclid else _gen(8, 4, dim)
    for n in (1, 2, 127, 128, 129, k - 1, k, k + 1, 2047, 2048, 2049, 60_000):
        rows = big[:n]
        sh = _shard(S, rows, euclid)
        for kk in (k, 1):
            doc, score, cnt, tot = sh.search_vector_batch(qs, kk)
            _check(doc, score, cnt, rows, qs, kk, euclid, O=O, ctx="n %d k %d" % (n, kk))
        sh.close()


@pytest.mark.parametrize("euclid", [False, True])
def test_batch_seams(S, O, euclid):
    """1, 31, 32, 33, 63, 64, 65 and 129 queries per call (the TWO half at 32, SS_VEC_BATCH at 64): every query gets the answer it
    gets alone"""
    n, dim, k = 6000, 96, 20
    rows = naive.vec_offcentre(11, n, dim, 10.0, 1.0) if euclid else _gen(11, n, dim, 3.0)
    qs = naive.vec_offcentre(12, 129, dim, 10.0, 1.0) if euclid else _gen(12, 129, dim, 3.0)
    sh = _shard(S, rows, euclid)
    alone = [sh.search_vector_batch(qs[i:i + 1], k) for i in range(129)]
    for i in range(0, 129, 16):
        _check(alone[i][0], alone[i][1], alone[i][2], rows, qs[i:i + 1], k, euclid, O=O, ctx="alone %d" % i)
    for nq in (1, 31, 32, 33, 63, 64, 65, 129):
        doc, score, cnt, _ = sh.search_vector_batch(qs[129 - nq:], k)
        for j in range(nq):
            a = alone[129 - nq + j]
            assert cnt[j] == a[2][0] and np.array_equal(doc[j], a[0][0]) and np.array_equal(score[j], a[1][0]), (nq, j)
    sh.close()


# ---------------------------------------------------------------- k at SS_MAX_K
def test_k_max_ties_through_every_chunk_seam(S):
    """an all-equal image of 40 000 rows at k = 1024: rows 0 .. 1023, whatever chunk they were scanned in; then 3 records per doc:
    docs 0 .. 1023, each once; Euclidean: every distance 0"""
    n, dim = 40_000, 16
    rows = np.tile(np.linspace(-1, 1, dim, dtype=np.float32), (n, 1))
    q = np.linspace(1, 2, dim, dtype=np.float32)[None, :]
    for euclid in (False, True):
        sh = _shard(S, rows, euclid)
        doc, score, cnt, _ = sh.search_vector_batch(np.vstack([q, rows[:1]]), MAX_K)
        assert list(cnt) == [MAX_K, MAX_K]
        for i in range(2):
            assert list(doc[i]) == list(range(MAX_K)) and np.all(score[i] == score[i][0]), (euclid, i)
        assert not euclid or np.all(score[1] == 0.0)
        sh.close()
        sh = _shard(S, rows, euclid, row_doc=(np.arange(n) // 3).astype(np.uint32))
        doc, score, cnt, _ = sh.search_vector_batch(q, MAX_K)
        assert cnt[0] == MAX_K and list(doc[0]) == list(range(MAX_K)), euclid
        sh.close()


@pytest.mark.parametrize("euclid", [False, True])
def test_k_max_adversarial_order(S, O, euclid):
    """rows in ascending order of similarity: every chunk's rows beat the last chunk's k-th, the candidate slots overflow and the
    batch runs again in safe mode (56-tile steps at k = 1024); k past the row count returns every row"""
    n, dim = 30_000, 24
    rng = np.random.default_rng(21)
    q = (rng.random(dim) + 0.5).astype(np.float32)
    t = np.linspace(0.0, 1.0, n)
    if euclid:
        rows = (q[None, :] + np.outer(1.0 - t, np.ones(dim)) * 5.0 + rng.standard_normal((n, dim)) * 0.01).astype(np.float32)
    else:
        rows = (np.outer(t, q) + rng.standard_normal((n, dim)) * 0.01).astype(np.float32)
    sh = _shard(S, rows, euclid)
    qs = np.vstack([q, q * np.float32(0.5)])
    doc, score, cnt, _ = sh.search_vector_batch(qs, MAX_K)
    _check(doc, score, cnt, rows, qs, MAX_K, euclid, O=O, ctx="adversarial")
    sh.close()
    small = rows[:700]
    sh = _shard(S, small, euclid)
    doc, score, cnt, _ = sh.search_vector_batch(qs, MAX_K)
    assert list(cnt) == [700, 700]
    _check(doc, score, cnt, small, qs, MAX_K, euclid, O=O, ctx="k > rows")
    sh.close()


# ---------------------------------------------------------------- values
def test_dot_values(S):
    """wide dynamic range (|x|, |q| <= 1e15), every score negative (no threshold), scores that cancel to near 0 -- where a relative
    tolerance sees nothing -- all under bound_dot"""
    n, dim = 5000, 64
    rng = np.random.default_rng(31)
    wide = (rng.standard_normal((n, dim)) * 10.0 ** rng.uniform(-12, 14, (n, 1))).astype(np.float32)
    wq = (rng.standard_normal((3, dim)) * 10.0 ** rng.uniform(-3, 1, (3, 1))).astype(np.float32)
    neg = -np.abs(_gen(32, n, dim))
    nq = np.abs(_gen(33, 3, dim))
    # cancellation: x = [a, -a * r + e] against q = [r, 1] (elementwise): x . q = e . 1, tiny beside sum |x q|
    a = _gen(34, n, dim // 2, 100.0)
    r = (np.random.default_rng(35).random(dim // 2) + 0.5).astype(np.float32)
    e = _gen(36, n, dim // 2, 1e-3)
    canc = np.hstack([a, (-a * r + e).astype(np.float32)])
    cq = np.hstack([r, np.ones(dim // 2, np.float32)])[None, :]
    for rows, qs in ((wide, wq), (neg, nq), (canc, cq)):
        sh = _shard(S, rows, False)
        for k in (10, 500):
            doc, score, cnt, _ = sh.search_vector_batch(qs, k)
            _check(doc, score, cnt, rows, qs, k, False)
        if rows is neg:
            assert np.all(score[:, :int(cnt[0])] < 0)
        sh.close()


@pytest.mark.parametrize("euclid", [False, True])
def test_threshold_on_a_score_and_tombstones_at_the_ends(S, O, euclid):
    """a similarity threshold equal to a returned score keeps that record (`score < threshold -> reject`); tombstones at row 0 and
    at the last row are never returned"""
    n, dim, k = 3000, 48, 50
    rows = naive.vec_offcentre(41, n, dim, 50.0, 0.2) if euclid else _gen(41, n, dim)
    qs = np.vstack([rows[0], rows[n - 1], naive.vec_offcentre(42, 1, dim, 50.0, 0.2) if euclid else _gen(42, 1, dim)])
    sh = _shard(S, rows, euclid)
    if euclid:  # Euclidean scores are the reference's own: the threshold falls exactly on one, and on the oracle's
        doc, score, cnt, _ = sh.search_vector_batch(qs[2:], k)
        for j in (0, 7, 20):
            t = -float(score[0][j])  # (a Euclidean threshold is a squared distance)
            d3, s3, c3, _ = sh.search_vector_batch(qs[2:], k, similarity_threshold=t)
            od, os_, *_ = O.vec_search_euclid(rows, qs[2], k, threshold_raw=np.float32(-t))
            assert int(c3[0]) == len(od) >= j + 1 and np.array_equal(s3[0][:int(c3[0])], os_)
            assert set(d3[0][:int(c3[0])].tolist()) == set(od.tolist())
    sh.set_deleted([0, n - 1])
    live = np.ones(n, bool)
    live[[0, n - 1]] = False
    doc, score, cnt, _ = sh.search_vector_batch(qs, k)
    _check(doc, score, cnt, rows, qs, k, euclid, live=live, O=O, ctx="tombstones")
    sh.close()


# ---------------------------------------------------------------- i8
def _i8_equal(doc, score, cnt, od, os_, every=None):
    """scores == the oracle's; the same rows above the k-th score; among rows tied AT the k-th score the reference keeps whichever
    its TopK slots happen to hold (vector.rs:461-487), this scan the lowest rows: with `every` (the f32 score of
    every row) the whole list must be (score desc, row asc)"""
    n = int(cnt)
    assert n == len(od) and np.array_equal(score[:n], os_)
    if n:
        assert set(doc[:n][score[:n] > os_[-1]].tolist()) == set(od[os_ > os_[-1]].tolist())
    d = doc[:n].astype(np.int64)
    assert np.all(np.diff(d)[np.diff(score[:n]) == 0] > 0), "equal scores out of row order"
    if every is not None:
        assert np.array_equal(d, np.lexsort((np.arange(len(every)), -np.asarray(every, np.float64)))[:n])


@pytest.mark.parametrize("dim", [1, 127, 129, 200, 2048])
def test_i8_extremes(S, O, dim):
    """every component -128 or 127: integer dots, == with the oracle, ties in row order"""
    n, k = 3000, 100
    rng = np.random.default_rng(dim)
    rows = np.where(rng.random((n, dim)) < 0.5, -128, 127).astype(np.int8)
    qs = np.where(rng.random((4, dim)) < 0.5, -128, 127).astype(np.int8)
    qs[0] = 127
    sh = S.Shard(0)
    sh.upload_vectors_i8(rows)
    doc, score, cnt, _ = sh.search_vector_batch_i8(qs, k)
    for i in range(len(qs)):
        od, os_, *_ = O.vec_search_i8(rows, qs[i], k)
        _i8_equal(doc[i], score[i], cnt[i], od, os_, (rows.astype(np.int64) @ qs[i].astype(np.int64)).astype(np.float32))
    sh.close()
    # Euclidean, plain and quantised (scales, norms) at the same extremes
    sh = S.Shard(0)
    sh.set_vector_similarity("euclidean")
    sh.upload_vectors_i8(rows)
    doc, score, cnt, _ = sh.search_vector_batch_i8(qs, k)
    for i in range(len(qs)):
        od, os_, *_ = O.vec_search_i8_euclid(rows, qs[i], k)
        d2 = ((rows.astype(np.int64) - qs[i].astype(np.int64)) ** 2).sum(axis=1)
        _i8_equal(doc[i], score[i], cnt[i], od, os_, -d2.astype(np.float32))
    rs = (rng.random(n) * 0.01 + 0.001).astype(np.float32)
    rn = (rng.random(n) * 50 + 1).astype(np.float32)
    qsc = (rng.random(len(qs)) * 0.01 + 0.001).astype(np.float32)
    qn = (rng.random(len(qs)) * 50 + 1).astype(np.float32)
    sh.upload_vectors_i8(rows, row_scale=rs)
    sh.set_row_norms(rn)
    doc, score, cnt, _ = sh.search_vector_batch_i8(qs, k, query_scale=qsc, query_norm=qn)
    for i in range(len(qs)):
        od, os_, *_ = O.vec_search_i8_euclid(rows, qs[i], k, row_scale=rs, row_norm=rn, query_scale=float(qsc[i]), query_norm=float(qn[i]))
        _i8_equal(doc[i], score[i], cnt[i], od, os_)
    sh.close()


def test_i8_dots_past_2_24_round_to_ties(S, O):
    """|dot| > 2^24: the integer dots 33 016 063 + v (v = -128 .. 127) meet in pairs on one f32; the reference compares the f32
    values, so of two rows that tie there the lower one wins -- at the k-th place too"""
    dim = 2048
    v = np.random.default_rng(51).permutation(np.arange(-128, 128))
    rows = np.full((256, dim), 127, np.int8)
    rows[:, -1] = v.astype(np.int8)
    q = np.full((1, dim), 127, np.int8)
    q[0, -1] = 1
    assert 127 * 127 * 2047 + 127 > 2 ** 24
    sh = S.Shard(0)
    sh.upload_vectors_i8(rows)
    for k in (1, 7, 64, 255):
        doc, score, cnt, _ = sh.search_vector_batch_i8(q, k)
        od, os_, *_ = O.vec_search_i8(rows, q[0], k)
        _i8_equal(doc[0], score[0], cnt[0], od, os_, (rows.astype(np.int64) @ q[0].astype(np.int64)).astype(np.float32))
        assert len(set(score[0][:k].tolist())) < k or k == 1
    sh.close()


# ---------------------------------------------------------------- f32 Euclidean off the origin
OFF = [(10.0, 1.0), (100.0, 0.1), (30.0, 0.01), (1000.0, 1.0), (1000.0, 0.1)]


@pytest.fixture(scope="module")
def offworld():
    """20 000 x 128 rows around each centre, 6 queries drawn the same way and 2 that are a row plus a tiny perturbation"""
    out = {}
    for c, s in OFF:
        rows = naive.vec_offcentre(61, 20_000, 128, c, s)
        qs = naive.vec_offcentre(62, 6, 128, c, s)
        pert = (rows[[5, 19_999]] + np.float32(s * 1e-3) * _gen(63, 2, 128)).astype(np.float32)
        out[(c, s)] = (rows, np.vstack([qs, pert]))
    return out


@pytest.mark.parametrize("c,sigma", OFF)
def test_euclidean_off_centre_all(S, O, offworld, c, sigma):
    rows, qs = offworld[(c, sigma)]
    sh = _shard(S, rows, True)
    for k in (10, 100):
        doc, score, cnt, _ = sh.search_vector_batch(qs, k)
        _check(doc, score, cnt, rows, qs, k, True, O=O, ctx="c %g sigma %g k %d" % (c, sigma, k))
    doc, score, cnt, _ = sh.search_vector_batch(qs[:2], 2300)  # one deep page
    _check(doc, score, cnt, rows, qs[:2], 2300, True, ctx="deep page")
    sh.close()
    # several records per doc: a doc's best record by exact distance
    ids = (np.arange(len(rows)) // 3).astype(np.uint32)
    sh = _shard(S, rows, True, row_doc=ids)
    doc, score, cnt, _ = sh.search_vector_batch(qs, 50)
    _check(doc, score, cnt, rows, qs, 50, True, row_doc=ids, ctx="3 records per doc")
    sh.close()


def _selected_rows(rows, q, lc, child, n_probe, euclid):
    """rows of the clusters AnnMode::Nprobe visits: per level, the n_probe clusters whose medoid (first record) scores best"""
    live = np.zeros(len(rows), bool)
    r0, ci = 0, 0
    for C in lc:
        starts, r = [], r0
        for j in range(C):
            starts.append(r)
            r += child[ci + j]
        med = rows[starts]
        sc = _exact(med, q, euclid)[0]
        for j in sorted(range(C), key=lambda j: (-sc[j], j))[:n_probe]:
            live[starts[j]:starts[j] + child[ci + j]] = True
        r0, ci = r, ci + C
    return live


@pytest.mark.parametrize("c,sigma", [(100.0, 0.1), (1000.0, 1.0)])
def test_euclidean_off_centre_nprobe(S, O, offworld, c, sigma):
    """AnnMode::Nprobe over two levels of clusters that end mid-tile"""
    rows, qs = offworld[(c, sigma)]
    lc = [6, 5]
    child = [1000, 2500, 1777, 3000, 1300, 1423, 1600, 2000, 2100, 1500, 1800]
    assert sum(child) == len(rows)
    sh = _shard(S, rows, True)
    sh.set_clusters(lc, child)
    doc, score, cnt, _, ncl = sh.search_vector_batch(qs, 30, ann_mode=S.AnnMode.Nprobe(2), with_clusters=True)
    for i in range(len(qs)):
        live = _selected_rows(rows, qs[i], lc, child, 2, True)
        *_, oncl = O.vec_search_euclid(rows, qs[i], 30, lc, child, n_probe=2)
        assert ncl[i] == oncl == 4
        _check(doc[i:i + 1], score[i:i + 1], cnt[i:i + 1], rows, qs[i:i + 1], 30, True, live=live, O=O, ctx="nprobe")
    sh.close()


@pytest.mark.parametrize("c,sigma", [(100.0, 0.1), (30.0, 0.01)])
def test_euclidean_off_centre_index_two_shards(S, O, offworld, c, sigma):
    """Index.search over 2 shards (doc g in shard g % 2), SearchMode.Vector: the global exact top 10"""
    rows, qs = offworld[(c, sigma)]
    shards = [_shard(S, rows[sid::2], True, shard_id=sid) for sid in range(2)]
    idx = S.Index(shards)
    for i in range(len(qs)):
        ro = idx.search(None, qs[i], S.QueryType.Union, S.SearchMode.Vector, 0, 10, S.ResultType.TopkCount, normalize_query=False)
        d = np.array([r.doc_id for r in ro.results], np.int64)
        s = np.array([r.score for r in ro.results], np.float32)
        ex, bd = _exact(rows, qs[i], True)
        naive.check_vector_topk(d, s, len(d), ex, bd, 10)
    for sh in shards:
        sh.close()


def test_ann_sparse_instance(S):
    """Dot under Nprobe with more than 32 queries and dim % 256 == 0: the VALU instance (vec_ann_sparse_kernel), clusters that end
    mid-tile"""
    dim, nq, k = 256, 40, 25
    child = [300, 517, 129, 700, 255, 1000, 383, 640, 77, 999, 512, 488]
    rows = _gen(71, sum(child), dim)
    qs = _gen(72, nq, dim)
    sh = _shard(S, rows, False)
    sh.set_clusters([len(child)], child)
    doc, score, cnt, _, ncl = sh.search_vector_batch(qs, k, ann_mode=S.AnnMode.Nprobe(1), with_clusters=True)
    for i in range(nq):
        live = _selected_rows(rows, qs[i], [len(child)], child, 1, False)
        assert ncl[i] == 1
        _check(doc[i:i + 1], score[i:i + 1], cnt[i:i + 1], rows, qs[i:i + 1], k, False, live=live, ctx="sparse ann")
    sh.close()
