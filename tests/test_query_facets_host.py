"""query_facets on the host, no device: what a shard does to its raw facet counters (finish_facets, search.rs:3604-3760) and what
the planner does to the shards' maps (merge_facets, search.rs:1747-1870, 1929-1939, 2039-2048) -- the Python mirror and, through the
shim, the C++ mirror -- against a literal restatement of the crate's code written here.

Ties: the crate orders a hash map with an unstable sort, so among equal counts there is no reference order.  same_facet() therefore
compares the multiset of the returned counts, that every label strictly above the cut count is present with its count, and that labels
at the cut count come from the labels holding that count."""
import collections
import ctypes as C
import os

import numpy as np
import pytest

from seekstorm_amd.search import ResultType, finish_facets, merge_facets

U16_MAX = 0xFFFF
CAP_MANY = 0xFFFFFFFF
TYPE_CODE = {"u8": 0, "u16": 1, "u32": 2, "u64": 3, "i8": 4, "i16": 5, "i32": 6, "i64": 7, "f32": 8, "f64": 9, "string16": 10,
             "string32": 11, "stringset16": 10, "stringset32": 11, "point": 12}


# ------------------------------------------------------------------------------------------------ the crate, restated
def ref_shard_map(qf, counters, shard_number):
    """one facet of one shard: counters [n_buckets + 1] -> the crate's Vec<(String, usize)> as a list, or None when it inserts nothing.
    Returns (list whose ORDER among equal counts is arbitrary, cut) -- cut = how many entries the crate's take() keeps (None = all)."""
    values = {i: int(n) for i, n in enumerate(counters[:-1]) if int(n)}  # facet.values: only ids somebody counted into
    if qf["type"].startswith("string"):
        if int(qf["length"]) == 0 or not values:  # search.rs:3606
            return None
        if qf["type"].startswith("stringset"):
            hm = collections.Counter()
            for set_id, n in values.items():
                for term in qf["values"][set_id]:
                    hm[term] += n
            entries = list(hm.items())
        else:
            entries = [(qf["values"][i], n) for i, n in values.items()]
        entries = [(a, c) for a, c in entries if a.startswith(qf.get("prefix", ""))]
        facet_cap = 0 if shard_number == 1 else CAP_MANY  # search.rs:2466-2470
        return entries, max(int(qf["length"]), facet_cap)
    if not values:
        return None
    rt = qf.get("range_type", "within")
    if rt == "above":  # search.rs:3678-3688: by key descending, running sum
        s = 0
        for key in sorted(values, reverse=True):
            s += values[key]
            values[key] = s
    elif rt == "below":
        s = 0
        for key in sorted(values):
            s += values[key]
            values[key] = s
    listed = [(qf["ranges"][key][0], values[key]) for key in sorted(values)]  # by range index: an ORDERED list
    return [(a, c) for a, c in listed if a.startswith(qf.get("prefix", ""))], None  # search.rs:3752-3754


def ref_planner(query_facets, shard_lists, result_type):
    """shard_lists[s] = {field: [(label, count)]} as each shard returned it (already cut by the shard)"""
    if result_type == ResultType.Topk:
        return {}
    out = {}
    for qf in query_facets:
        summed = collections.Counter()
        for m in shard_lists:
            for label, n in m.get(qf["field"], []):
                summed[label] += n
        out[qf["field"]] = (dict(summed), U16_MAX if not qf["type"].startswith("string") else int(qf["length"]))
    return out


def same_facet(got, full, cut, what=""):
    """got: the list under test; full: {label: count} of everything eligible; cut: entries kept after ordering by count descending"""
    want_counts = sorted(full.values(), reverse=True)[:cut]
    assert sorted((c for _, c in got), reverse=True) == want_counts, (what, got, full, cut)
    assert len({a for a, _ in got}) == len(got), (what, "a label twice", got)
    assert [c for _, c in got] == sorted((c for _, c in got), reverse=True), (what, "not by count descending", got)
    if not want_counts:
        return
    cut_count = want_counts[-1]
    g = dict(got)
    for label, c in full.items():
        if c > cut_count:
            assert g.get(label) == c, (what, "missing above the cut", label, c)
    for label, c in got:
        assert full.get(label) == c, (what, "a count that is not the label's", label, c)


# ------------------------------------------------------------------------------------------------ the C++ mirror through the shim
def _spec(query_facets):
    lines = []
    for qf in query_facets:
        code = TYPE_CODE[qf["type"]]
        if not qf["type"].startswith("string"):
            base = qf.get("base", (0.0, 0.0))
            bits = _bounds_bits(qf)
            t = ["R", qf["field"], qf["offset"], code, {"within": 0, "above": 1, "below": 2}[qf.get("range_type", "within")], repr(float(base[0])),
                 repr(float(base[1])), {"km": 1, "miles": 2}[qf.get("unit", "km")], qf.get("prefix", ""), len(qf["ranges"])]
            for (label, _), b in zip(qf["ranges"], bits):
                t += [label, int(b)]
        elif qf["type"].startswith("stringset"):
            t = ["T", qf["field"], qf["offset"], code, qf.get("prefix", ""), qf["length"], len(qf["values"])]
            for members in qf["values"]:
                t += [len(members)] + list(members)
        else:
            t = ["S", qf["field"], qf["offset"], code, qf.get("prefix", ""), qf["length"], len(qf["values"])] + list(qf["values"])
        lines.append("\t".join(str(x) for x in t))
    return "\n".join(lines).encode()


def _bounds_bits(qf):
    lows = [b for _, b in qf["ranges"]]
    if qf["type"] in ("f64", "point"):
        return np.asarray(lows, np.float64).view(np.uint64)
    if qf["type"] == "f32":
        return np.asarray(lows, np.float32).view(np.uint32).astype(np.uint64)
    return np.array([int(x) & 0xFFFFFFFFFFFFFFFF for x in lows], np.uint64)


def parse_facets_text(text):
    out = {}
    for line in text.split("\n"):
        if not line:
            continue
        t = line.split("\t")
        out.setdefault(t[0], [])
        if len(t) == 3:
            out[t[0]].append((t[1], int(t[2])))
    return out


_HOST = None


def host_lib():
    global _HOST
    if _HOST is None:
        import seekstorm_amd
        path = os.path.join(os.path.dirname(seekstorm_amd.__file__), "lib", "libseekstorm_host.so")
        L = C.CDLL(path)
        L.ssh_facets_finish.restype = C.c_int
        L.ssh_facets_finish.argtypes = [C.c_char_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_int, C.c_uint32, C.c_char_p, C.c_uint32]
        _HOST = L
    return _HOST


def cpp_finish(query_facets, shard_counts, shard_number, merge, result_type=ResultType.TopkCount):
    """shard_counts[s][f] = counters of facet f in shard s"""
    flat = np.concatenate([np.concatenate([np.asarray(c, np.uint64) for c in per]) for per in shard_counts])
    buf = C.create_string_buffer(1 << 16)
    n = host_lib().ssh_facets_finish(_spec(query_facets), len(shard_counts), flat.ctypes.data, shard_number, 1 if merge else 0, int(result_type), buf,
                                     len(buf))
    assert n >= 0, n
    return parse_facets_text(buf.value.decode())


def py_finish(query_facets, shard_counts, shard_number, merge, result_type=ResultType.TopkCount):
    maps = [finish_facets(query_facets, per, shard_number) for per in shard_counts]
    return merge_facets(query_facets, maps, result_type) if merge else maps[0]


MIRRORS = [("python", py_finish), ("c++", cpp_finish)]


def _check_shard(finish, query_facets, counts, shard_number):
    got = finish(query_facets, [counts], shard_number, False)
    for qf, c in zip(query_facets, counts):
        ref = ref_shard_map(qf, c, shard_number)
        if ref is None or not ref[0]:
            assert qf["field"] not in got, (qf["field"], got)
            continue
        entries, cut = ref
        if qf["type"].startswith("string"):
            same_facet(got[qf["field"]], dict(entries), cut, qf["field"])
        else:
            assert got[qf["field"]] == entries, (qf["field"], got[qf["field"]], entries)  # by range index: an exact list
    return got


RANGES = [("0-9", 0), ("10-99", 10), ("100-999", 100), ("1000-", 1000), ("huge", 1 << 40)]


def _range_facet(rt, field="price", ty="u64", prefix=""):
    return {"field": field, "offset": 0, "type": ty, "ranges": RANGES, "range_type": rt, "prefix": prefix}


@pytest.mark.parametrize("mirror,finish", MIRRORS)
def test_the_three_range_types_with_empty_ranges(mirror, finish):
    """within / above / below on hand-made counters; ranges nobody fell into have no entry and take no part in the running sums' keys;
    the "other" slot is dropped"""
    counts = [7, 0, 5, 0, 2, 99]  # ranges 1 and 3 empty, 99 docs outside
    for rt, want in (("within", [("0-9", 7), ("100-999", 5), ("huge", 2)]), ("above", [("0-9", 14), ("100-999", 7), ("huge", 2)]),
                     ("below", [("0-9", 7), ("100-999", 12), ("huge", 14)])):
        got = _check_shard(finish, [_range_facet(rt)], [counts], 1)
        assert got == {"price": want}, (mirror, rt, got)
    assert finish([_range_facet("above")], [[[0, 0, 0, 0, 0, 5]]], 1, False) == {}  # nobody inside a range: the facet is left out
    # a float facet and a Point facet finish the same way; a prefix filters range labels too (search.rs:3752-3754)
    f = {"field": "d", "offset": 8, "type": "point", "ranges": [("near", 0.0), ("mid", 100.0), ("far", 1000.0)], "range_type": "below",
         "base": (38.9, -77.0), "unit": "miles"}
    assert _check_shard(finish, [f], [[1, 2, 3, 0]], 1) == {"d": [("near", 1), ("mid", 3), ("far", 6)]}
    assert _check_shard(finish, [_range_facet("within", prefix="10")], [counts], 1) == {"price": [("100-999", 5)]}


VALUES = ["apple", "apricot", "banana", "blueberry", "cherry", "avocado", "almond", "beet"]


def _string_facet(length, prefix="", ty="string16"):
    return {"field": "fruit", "offset": 4, "type": ty, "values": VALUES, "prefix": prefix, "length": length}


@pytest.mark.parametrize("mirror,finish", MIRRORS)
def test_prefix_and_length(mirror, finish):
    counts = [5, 9, 9, 1, 0, 9, 3, 2, 40]  # three values tie at 9; cherry empty; 40 outside the table
    for length in (0, 1, 2, 3, 4, 7, 8, 100):
        for prefix in ("", "a", "b", "ap", "zz"):
            _check_shard(finish, [_string_facet(length, prefix)], [counts], 1)
    got = finish([_string_facet(2, "a")], [[counts]], 1, False)["fruit"]
    assert sorted(c for _, c in got) == [9, 9] and {a for a, _ in got} == {"apricot", "avocado"}  # prefix first, then take(length)
    assert finish([_string_facet(0)], [[counts]], 1, False) == {} and finish([_string_facet(3, "zz")], [[counts]], 1, False) == {}
    assert finish([_string_facet(3)], [[[0] * 8 + [12]]], 1, False) == {}  # a facet nobody counted into


@pytest.mark.parametrize("mirror,finish", MIRRORS)
def test_cap_for_one_shard_and_for_two(mirror, finish):
    """take(max(length, cap)): one shard cuts to length, a shard of several returns everything (the planner cuts)"""
    counts = [5, 9, 9, 1, 4, 9, 3, 2, 0]
    one = _check_shard(finish, [_string_facet(3)], [counts], 1)["fruit"]
    two = _check_shard(finish, [_string_facet(3)], [counts], 2)["fruit"]
    assert len(one) == 3 and len(two) == 8
    assert dict(two) == dict(zip(VALUES, counts[:8]))


@pytest.mark.parametrize("mirror,finish", MIRRORS)
def test_stringset_expansion_where_two_sets_share_a_member(mirror, finish):
    sets = [["red"], ["red", "green"], ["green", "blue"], [], ["blue"]]
    qf = {"field": "colour", "offset": 2, "type": "stringset16", "values": sets, "prefix": "", "length": 10}
    counts = [4, 10, 3, 8, 0, 6]  # the empty set's 8 docs reach no string; set 4 is empty of docs
    got = _check_shard(finish, [qf], [counts], 1)["colour"]
    assert dict(got) == {"red": 14, "green": 13, "blue": 3}
    qf2 = dict(qf, type="stringset32", length=1, prefix="")
    assert _check_shard(finish, [qf2], [counts], 1)["colour"] == [("red", 14)]
    assert _check_shard(finish, [dict(qf, prefix="g")], [counts], 1)["colour"] == [("green", 13)]


@pytest.mark.parametrize("mirror,finish", MIRRORS)
def test_topk_drops_the_facets(mirror, finish):
    qfs = [_string_facet(3), _range_facet("within")]
    counts = [[5, 9, 9, 1, 4, 9, 3, 2, 0], [7, 0, 5, 0, 2, 9]]
    assert finish(qfs, [counts, counts], 2, True, ResultType.Topk) == {}
    for rt in (ResultType.TopkCount, ResultType.Count):
        assert set(finish(qfs, [counts, counts], 2, True, rt)) == {"fruit", "price"}


@pytest.mark.parametrize("mirror,finish", MIRRORS)
def test_two_shard_sum_and_the_second_cut(mirror, finish):
    """the planner sums the shards' maps by key, orders by count and cuts to the facet's length -- range facets to u16::MAX, by count too"""
    rng = np.random.default_rng(5)
    for trial in range(30):
        length = int(rng.integers(1, 9))
        prefix = ["", "a", "b"][trial % 3]
        qfs = [_string_facet(length, prefix), _range_facet(["within", "above", "below"][trial % 3]),
               {"field": "colour", "offset": 2, "type": "stringset32", "values": [["red"], ["red", "green"], ["green", "blue"]], "prefix": "", "length": 2}]
        shard_counts = [[rng.integers(0, 4, 9) * rng.integers(0, 2, 9), rng.integers(0, 5, 6) * rng.integers(0, 2, 6), rng.integers(0, 6, 4)] for _ in range(2)]
        got = finish(qfs, shard_counts, 2, True)
        shard_lists = []
        for per in shard_counts:
            m = {}
            for qf, c in zip(qfs, per):
                ref = ref_shard_map(qf, c, 2)
                if ref is not None and ref[0]:
                    m[qf["field"]] = ref[0]  # (cap unlimited for two shards: nothing is cut by the shard)
            shard_lists.append(m)
        want = ref_planner(qfs, shard_lists, ResultType.TopkCount)
        assert set(got) == set(want), (mirror, trial)
        for field, (full, cut) in want.items():
            same_facet(got[field], full, cut, (mirror, trial, field))
    # the second cut by hand: shard A {x: 3, y: 2}, shard B {y: 2, z: 3}, length 2 -> y (4) and one of x / z (3)
    qf = {"field": "f", "offset": 0, "type": "string32", "values": ["x", "y", "z"], "prefix": "", "length": 2}
    got = finish([qf], [[[3, 2, 0, 0]], [[0, 2, 3, 0]]], 2, True)["f"]
    assert got[0] == ("y", 4) and got[1] in (("x", 3), ("z", 3)) and len(got) == 2
    # a facet nobody counted into still has its (empty) entry in the planner's map (search.rs:1749-1870 inserts every requested facet)
    assert finish([qf], [[[0, 0, 0, 5]], [[0, 0, 0, 1]]], 2, True) == {"f": []}


def test_result_object_has_facets():
    from seekstorm_amd.search import ResultObject
    assert ResultObject().facets == {}


def test_query_facets_are_refused_where_they_would_be_dropped():
    """Index.search: query_facets with a result_sort, a vector-only search or no terms raise instead of returning no facets"""
    from seekstorm_amd.search import Index, SearchMode
    qf = [_range_facet("within")]
    ix = Index([])
    with pytest.raises(ValueError):
        ix.search([1, 2], query_facets=qf, result_sort=[(0, "u32", False)])
    with pytest.raises(ValueError):
        ix.search([1, 2], query_vector=np.zeros(4, np.float32), search_mode=SearchMode.Vector, query_facets=qf)
    with pytest.raises(ValueError):
        ix.search([], query_facets=qf)
    ix.search([1, 2], query_facets=qf)  # (a lexical search by score takes them)
