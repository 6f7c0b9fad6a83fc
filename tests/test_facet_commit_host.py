"""The facet commit seam without a device: argument checks of the new entry points, the Rust FFI, and the rank tables of the two
mirrors (CPU)."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ["ss_facet_append_level", "ss_facet_reserve", "ss_facet_info", "ss_facet_set_string_ranks", "ss_facet_string_ranks",
               "ss_add_deleted"]
WORDS = ["zeta", "alpha", "Alpha", "beta", "éclair", "eclair", "omega", "beta", "a", "", "zz", "中文", "alpha ", "b", "B", "beta"]


def test_new_entry_points_refuse_missing_arguments():
    """no shard / no arrays -> SS_EINVAL (-1), before a device is touched (this machine has none)"""
    from seekstorm_amd import _native as N
    L = N.lib()
    rec = np.zeros((4, 8), np.uint8)
    ids = np.zeros(4, np.uint32)
    out = np.zeros(4, np.uint32)
    d64 = np.zeros(4, np.uint64)
    s16 = N.FACET_TYPES["string16"]
    assert L.ss_facet_append_level(None, 0, 4, 8, N.ptr(rec, N.u8p)) == -1
    assert L.ss_facet_reserve(None, 100) == -1
    assert L.ss_facet_info(None, None, None, None, None) == -1
    assert L.ss_facet_set_string_ranks(None, 0, s16, 4, N.ptr(ids, N.u32p)) == -1
    assert L.ss_facet_set_string_ranks(None, 0, s16, 0, None) == -1
    assert L.ss_facet_string_ranks(None, 4, N.ptr(ids, N.u32p), 0, s16, N.ptr(out, N.u32p)) == -1
    assert L.ss_add_deleted(None, N.ptr(d64, N.u64p), 4) == -1
    assert L.ss_add_deleted(None, None, 0) == -1


def test_header_ffi_and_bindings_name_every_new_entry():
    from seekstorm_amd import _native as N
    hdr = open(os.path.join(ROOT, "include", "seekstorm_hip.h")).read()
    ffi = open(os.path.join(ROOT, "integration", "hip_ffi.rs")).read()
    bound = {s[0] for s in N.SYMBOLS}
    for name in NEW_ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert re.search(r"\bfn\s+%s\s*\(" % name, ffi), name
        assert name in bound, name
    assert int(re.search(r"#define\s+SS_MAX_STRING_RANKS\s+(\d+)", hdr).group(1)) == N.SS_MAX_STRING_RANKS == 8
    assert int(re.search(r"#define\s+SS_ABI_VERSION\s+(\d+)", hdr).group(1)) == 7  # additive: the ABI version stays


def _cpp_ranks(words):
    import seekstorm_amd
    H = C.CDLL(os.path.join(os.path.dirname(seekstorm_amd.__file__), "lib", "libseekstorm_host.so"))
    H.ssh_string_ranks.restype = None
    H.ssh_string_ranks.argtypes = [C.c_char_p, C.c_uint64, C.c_uint32, C.c_void_p]
    buf = b"\0".join(w.encode("utf-8") for w in words)
    out = np.zeros(len(words), np.uint32)
    H.ssh_string_ranks(buf, len(buf), len(words), out.ctypes.data)
    return out


def test_rank_tables_of_the_two_mirrors_agree():
    """rank[id] = the rank of the id's string in byte-wise UTF-8 order, equal strings sharing a rank: Python's Shard.string_ranks, the
    C++ mirror's string_ranks and a plain statement of the rule"""
    import seekstorm_amd as S
    keys = [w.encode("utf-8") for w in WORDS]
    want = np.array([sorted(set(keys)).index(kb) for kb in keys], np.uint32)
    py = S.Shard.string_ranks(WORDS)
    assert py.dtype == np.uint32 and np.array_equal(py, want)
    assert np.array_equal(_cpp_ranks(WORDS), want)
    # equal strings share a rank; the order is that of the bytes, not of the code points' case folding or the locale
    assert want[3] == want[7] == want[15] and want[9] == 0
    assert want[WORDS.index("B")] < want[WORDS.index("a")] < want[WORDS.index("alpha")] < want[WORDS.index("alpha ")] < want[WORDS.index("b")]
    assert want[WORDS.index("zz")] < want[WORDS.index("éclair")] < want[WORDS.index("中文")]
    # ranked in a wider order (the union of several shards' strings): ranks of that order, still shared by equal strings
    order = sorted(set(keys) | {b"aardvark", b"zzz"})
    wide = S.Shard.string_ranks(WORDS, order)
    assert np.array_equal(wide, np.array([order.index(kb) for kb in keys], np.uint32))
    assert S.Shard.string_ranks([]).shape == (0,)


def test_index_ranks_come_from_one_order_over_all_shards():
    """Index.set_string_facet_ranks: the tables of the shards, captured without a device"""
    import seekstorm_amd as S
    calls = []

    class Capture(S.Shard):
        def __init__(self, sid):  # no device
            self.sid = sid

        def set_string_facet_ranks(self, facet_offset, facet_type, strings, order=None):
            calls.append((self.sid, facet_offset, facet_type, S.Shard.string_ranks(strings, order).tolist()))

        def __del__(self):
            pass

    idx = S.Index([Capture(0), Capture(1)])
    idx.set_string_facet_ranks(6, "string16", [["b", "a", "d"], ["c", "a"]])
    assert calls == [(0, 6, "string16", [1, 0, 3]), (1, 6, "string16", [2, 0])]
