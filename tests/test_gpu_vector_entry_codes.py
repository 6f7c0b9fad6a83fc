"""Return codes of the ten vector search entries, host- and device-pointer, for bad inputs alone and in pairs (csrc/api_vec.hip; -m gpu).

ss_vec_search[_ann], ss_vec_search_i8[_ann | _euclid] and their _dev forms check their arguments, the image and the ANN mode in an order
that is part of their behaviour: null pointers, k = 0, the image of the entry's kind, for i8 the norms a Euclidean image with scales
needs, then the mode (a NaN threshold, clusters, field ids).  One table of rows (ROWS), every row an override of an entry's valid call;
every row alone and every pair of rows goes to every entry the rows apply to, and the code is compared with a literal.  The literals
(CODES) are the codes commit 3d35de9 returns: read off the order of its checks first, then confirmed by running this test against a
build of that commit.  No row or pair is accepted by the library and every refusal comes from a host-side check: no refused call
reaches a kernel.

The world: 300 rows x dim 24 (neither the row tile nor the padded width is met exactly), 3 queries, k = 5.  Shards: `f32`; `i8dot` (i8
rows with record scales, Dot); `i8e` / `i8e_bare` (i8 rows with record scales, Euclidean, with / without record norms); `clustered`
(the f32 rows in two clusters), which the valid calls under a mode that skips clusters go to; `empty`."""

import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_ROWS, DIM, NQ, K = 300, 24, 3, 5
LETTER = {0: "K", -1: "I", -2: "M", -3: "D", -4: "N", -5: "S"}  # OK, EINVAL, ENOMEM, EDEVICE, ENOTSUP, ESTATE
OUTS = "out_doc out_score out_count out_total"

# the C entry and its parameters in order
ENTRY = {
    "search": ("ss_vec_search", "shard nq queries k thr " + OUTS),
    "ann": ("ss_vec_search_ann", "shard nq queries k thr mode " + OUTS + " out_clusters"),
    "i8": ("ss_vec_search_i8", "shard nq queries qscale k thr " + OUTS),
    "i8_ann": ("ss_vec_search_i8_ann", "shard nq queries qscale k thr mode " + OUTS + " out_clusters"),
    "i8_euclid": ("ss_vec_search_i8_euclid", "shard nq queries qscale qnorm k thr mode " + OUTS + " out_clusters"),
}
ENTRY.update({e + "_dev": (name + "_dev", params + " stream") for e, (name, params) in list(ENTRY.items())})
PARAMS = {e: set(p.split()) for e, (_, p) in ENTRY.items()}
I8 = {e for e in ENTRY if e.startswith("i8")}
EUCLID = {"i8_euclid", "i8_euclid_dev"}
MODE = ("n_probe", "cluster_threshold_raw", "field_mask")  # (the valid call has no mode; a row that sets one of these brings one)

# (name, the entries it goes to -- a set of names, or the parameters an entry must take --, the overrides as functions of the valid call)
ROWS = [
    ("null shard", set(), {"shard": lambda a: None}),
    ("null queries", set(), {"queries": lambda a: None}),
    ("null out_doc", set(), {"out_doc": lambda a: None}),
    ("null out_score", set(), {"out_score": lambda a: None}),
    ("null out_count", set(), {"out_count": lambda a: None}),
    ("null out_total", set(), {"out_total": lambda a: None}),
    ("k = 0", set(), {"k": lambda a: 0}),
    ("NaN cluster threshold", {"mode"}, {"cluster_threshold_raw": lambda a: float("nan")}),
    ("mode skips clusters, image without clusters", {"mode"}, {"n_probe": lambda a: 1}),
    ("field mask, image without field ids", {"mode"}, {"field_mask": lambda a: 1}),
    ("i8 Euclidean with scales, no record norms", I8, {"shard": lambda a: "i8e_bare"}),
    ("i8 Euclidean with scales, no query norm", {"qnorm"}, {"qnorm": lambda a: None}),
    ("i8 Euclidean with scales, an entry without a query norm", I8 - EUCLID, {"shard": lambda a: "i8e"}),
    ("image of the other kind", set(), {"shard": lambda a: "f32" if a["entry"] in I8 else "i8dot"}),
    ("empty shard", set(), {"shard": lambda a: "empty"}),
]


def _applies(row, entry):
    to = row[1]
    return entry in to if to and to <= set(ENTRY) else to <= PARAMS[entry]


# CODES[entry][i][j], i <= j, over the rows that go to the entry: the code of rows i and j together (i == j: row i alone) in LETTER's
# letters; '.': the two rows override the same argument.  The codes of 3d35de9; an entry and its _dev form share a table.
_F32 = [
    "IIIIIII..",  # null shard
    " IIIIIIII",  # null queries
    "  IIIIIII",  # null out_doc
    "   IIIIII",  # null out_score
    "    IIIII",  # null out_count
    "     IIII",  # null out_total
    "      III",  # k = 0
    "       S.",  # image of the other kind
    "        S",  # empty shard
]
_F32_ANN = [
    "IIIIIIIIII..",  # null shard
    " IIIIIIIIIII",  # null queries
    "  IIIIIIIIII",  # null out_doc
    "   IIIIIIIII",  # null out_score
    "    IIIIIIII",  # null out_count
    "     IIIIIII",  # null out_total
    "      IIIIII",  # k = 0
    "       IIISS",  # NaN cluster threshold
    "        SSSS",  # mode skips clusters, image without clusters
    "         SSS",  # field mask, image without field ids
    "          S.",  # image of the other kind
    "           S",  # empty shard
]
_I8 = [
    "IIIIIII....",  # null shard
    " IIIIIIIIII",  # null queries
    "  IIIIIIIII",  # null out_doc
    "   IIIIIIII",  # null out_score
    "    IIIIIII",  # null out_count
    "     IIIIII",  # null out_total
    "      IIIII",  # k = 0
    "       S...",  # i8 Euclidean with scales, no record norms
    "        I..",  # i8 Euclidean with scales, an entry without a query norm
    "         S.",  # image of the other kind
    "          S",  # empty shard
]
_I8_ANN = [
    "IIIIIIIIII....",  # null shard
    " IIIIIIIIIIIII",  # null queries
    "  IIIIIIIIIIII",  # null out_doc
    "   IIIIIIIIIII",  # null out_score
    "    IIIIIIIIII",  # null out_count
    "     IIIIIIIII",  # null out_total
    "      IIIIIIII",  # k = 0
    "       IIISISS",  # NaN cluster threshold
    "        SSSISS",  # mode skips clusters, image without clusters
    "         SSISS",  # field mask, image without field ids
    "          S...",  # i8 Euclidean with scales, no record norms
    "           I..",  # i8 Euclidean with scales, an entry without a query norm
    "            S.",  # image of the other kind
    "             S",  # empty shard
]
_I8_EUCLID = [
    "IIIIIIIIII.I..",  # null shard
    " IIIIIIIIIIIII",  # null queries
    "  IIIIIIIIIIII",  # null out_doc
    "   IIIIIIIIIII",  # null out_score
    "    IIIIIIIIII",  # null out_count
    "     IIIIIIIII",  # null out_total
    "      IIIIIIII",  # k = 0
    "       IIISISS",  # NaN cluster threshold
    "        SSSISS",  # mode skips clusters, image without clusters
    "         SSISS",  # field mask, image without field ids
    "          SS..",  # i8 Euclidean with scales, no record norms
    "           ISS",  # i8 Euclidean with scales, no query norm
    "            S.",  # image of the other kind
    "             S",  # empty shard
]
CODES = {"search": _F32, "ann": _F32_ANN, "i8": _I8, "i8_ann": _I8_ANN, "i8_euclid": _I8_EUCLID}
CODES.update({e + "_dev": t for e, t in list(CODES.items())})


@pytest.fixture(scope="module")
def S():
    import seekstorm_amd
    return seekstorm_amd


def N():
    from seekstorm_amd import _native
    return _native


class World:
    pass


@pytest.fixture(scope="module")
def W(S):
    import torch
    W = World()
    rng = np.random.default_rng(11)
    rows = rng.standard_normal((N_ROWS, DIM)).astype(np.float32)
    rows8 = rng.integers(-127, 128, (N_ROWS, DIM)).astype(np.int8)
    scale = rng.uniform(0.5, 1.5, N_ROWS).astype(np.float32)
    W.host = {"q32": rng.standard_normal((NQ, DIM)).astype(np.float32), "q8": rng.integers(-127, 128, (NQ, DIM)).astype(np.int8),
              "qscale": rng.uniform(0.5, 1.5, NQ).astype(np.float32), "qnorm": rng.uniform(1.0, 2.0, NQ).astype(np.float32),
              "out_doc": np.full((NQ, K), 0xA5A5A5A5, np.uint32), "out_score": np.full((NQ, K), -7.5, np.float32),
              "out_count": np.full(NQ, 0xA5A5A5A5, np.uint32), "out_total": np.full(NQ, 0xA5A5A5A5A5A5A5A5, np.uint64),
              "out_clusters": np.full(NQ, 0xA5A5A5A5, np.uint32)}
    dev = torch.device("cuda", 0)
    W.dev = {key: torch.from_numpy(x.view({np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}.get(x.dtype, x.dtype))).to(dev)
             for key, x in W.host.items()}
    W.shards = {}
    try:
        for name in ("empty", "f32", "i8dot", "i8e", "i8e_bare", "clustered"):
            sh = W.shards[name] = S.Shard(0)
            if name in ("f32", "clustered"):
                sh.upload_vectors(rows)
            if name == "clustered":
                sh.set_clusters([2], [N_ROWS // 2, N_ROWS - N_ROWS // 2])
            if name in ("i8e", "i8e_bare"):
                sh.set_vector_similarity("euclidean")
            if name in ("i8dot", "i8e", "i8e_bare"):
                sh.upload_vectors_i8(rows8, row_scale=scale)
            if name == "i8e":
                sh.set_row_norms(rng.uniform(1.0, 2.0, N_ROWS).astype(np.float32))
        torch.cuda.synchronize()
        yield W
    finally:
        for sh in W.shards.values():
            sh.close()


def valid(W, entry):
    """the arguments of the entry's valid call"""
    a = dict(W.dev if entry.endswith("_dev") else W.host)
    a.update(entry=entry, shard="i8e" if entry in EUCLID else "i8dot" if entry in I8 else "f32", nq=NQ, k=K, thr=N().FLT_MIN_NEG,
             queries=a["q8" if entry in I8 else "q32"], stream=None, n_probe=0, cluster_threshold_raw=N().FLT_MIN_NEG, field_mask=0)
    return a


def call(W, entry, rows=(), **over):
    """the entry under its valid call's arguments with the rows' overrides (and `over`) written over them -> the code"""
    n, a = N(), valid(W, entry)
    over.update({key: fn(a) for row in rows for key, fn in row[2].items()})
    a.update(over)
    a["mode"] = n.AnnModeC(a["n_probe"], a["cluster_threshold_raw"], a["field_mask"], 0, 0) if set(MODE) & set(over) else None
    name, params = ENTRY[entry]
    fn = getattr(n.lib(), name)
    args = []
    for p, t in zip(params.split(), fn.argtypes):
        v = a[p]
        if p == "shard":
            v = None if v is None else W.shards[v]._h
        elif isinstance(v, np.ndarray):
            v = v.ctypes.data if t is C.c_void_p else v.ctypes.data_as(t)
        elif isinstance(v, C.Structure):
            v = C.addressof(v)
        elif hasattr(v, "data_ptr"):
            v = v.data_ptr()
        args.append(v)
    return fn(*args)


def observe(W, entry):
    """the table of `entry` as the library answers it now, in CODES' form"""
    rows = [r for r in ROWS if _applies(r, entry)]
    table = []
    for i, ri in enumerate(rows):
        line = " " * i
        for j in range(i, len(rows)):
            if i != j and set(ri[2]) & set(rows[j][2]):
                line += "."
                continue
            rc = call(W, entry, (ri,) if i == j else (ri, rows[j]))
            assert rc != 0, (entry, ri[0], rows[j][0], "accepted")
            line += LETTER[rc]
        table.append(line)
    return [r[0] for r in rows], table


def outputs(W, entry):
    import torch
    if entry.endswith("_dev"):
        torch.cuda.synchronize()
        return {key: W.dev[key].cpu().numpy().copy() for key in W.dev if key.startswith("out_")}
    return {key: W.host[key].copy() for key in W.host if key.startswith("out_")}


@pytest.mark.parametrize("entry", list(ENTRY))
def test_codes_of_rows_and_pairs(W, entry):
    before = outputs(W, entry)
    names, got = observe(W, entry)
    print("\n%s = [\n%s\n]" % (entry, "\n".join('    "%s",  # %s' % (line, name) for line, name in zip(got, names))))
    want = CODES[entry]
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        for j in range(i, len(names)):
            assert g[j] == w[j], (entry, names[i], names[j], g[j], w[j])
    after = outputs(W, entry)
    assert all(np.array_equal(before[key], after[key]) for key in before), entry  # (a refused call writes nothing)


@pytest.mark.parametrize("entry", list(ENTRY))
def test_empty_and_empty_deep_calls_write_nothing(W, entry):
    """nq = 0 under valid arguments, at k and at a k beyond SS_MAX_K (a deep page of no queries): SS_OK, the output arrays untouched"""
    before = outputs(W, entry)
    for k in (K, N().SS_MAX_K + 1):
        assert call(W, entry, nq=0, k=k) == N().SS_OK, (entry, k)
    after = outputs(W, entry)
    assert all(np.array_equal(before[key], after[key]) for key in before), entry


# (last: the valid calls write the shared output arrays)
@pytest.mark.parametrize("entry", list(ENTRY))
def test_valid_calls(W, entry):
    import torch
    assert call(W, entry) == N().SS_OK, entry
    if "mode" in PARAMS[entry] and entry not in I8:  # a mode that skips clusters, on the image that has them; its NaN threshold is still refused
        assert call(W, entry, shard="clustered", n_probe=1) == N().SS_OK, entry
        assert call(W, entry, shard="clustered", n_probe=1, cluster_threshold_raw=float("nan")) == N().SS_EINVAL, entry
    torch.cuda.synchronize()
    cnt = outputs(W, entry)["out_count"]
    assert np.all(cnt.view(np.uint32) == K), (entry, cnt)  # (300 rows, no threshold: every query fills its k)
