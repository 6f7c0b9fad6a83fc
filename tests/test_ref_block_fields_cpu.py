"""The per-posting decoder of FIELD VECTORS that the host and the device decode kernels share (seekstorm_amd/csrc/ref_block_decode.h
rbd_field_vec) on the CPU: a stand-alone program (tests/ref_block_fields_check.cpp, its own main) is compiled with g++ under
AddressSanitizer and UBSan and decodes every case RANK BY RANK with rbd_doc + rbd_field_vec; the expected postings -- or the expected
refusal -- of every case are what the library's whole-block host decoder (ss_ref_decode_block_fields / _ngram) answers for the same bytes.

Cases, each for 2, 3, 5 and 8 indexed fields (field id bits 1, 2, 3, 3; 5 does not fill its bits) and for the longest field 0 and the
last one: only-longest vectors with counts of 1, 2 and 3 bytes; vectors of 2, 3 and all fields with tfs of every VINT size; every
embedded tag of both pointer sizes (0x8 .. 0xF, 0x10 .. 0x1F); the pivot at 0, in the middle and at the count; Array, Rle and Bitmap
containers; n-gram keys of 2 and 3 components, every component.  Corrupted copies: byte_array_len truncated at EVERY length, single
bytes flipped by a seeded generator and at every bit where the structure lies -- each must end in the host decoder's answer for those
bytes, and in no sanitizer report (the bytes behind byte_array_len are poisoned while a copy is decoded).

A second test covers the argument checks of ss_bm25_open_index_bin_levels_fields and ss_bm25_level_read_fields that need no device, and
that the header and the Rust binding name both."""
import ctypes as C
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

from oracle import ref_format as RF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLIPS = 32  # seeded single-byte flips per case
FIELD_COUNTS = (2, 3, 5, 8)


def _spaced(n, step=3, first=1):
    return [first + step * i for i in range(n)]


def _tags(body, ctp, cnt, pivot):
    """the embedded tags among a body's pointers: 2-byte pointers' bits 15 .. 12, 3-byte pointers' bits 23 .. 19"""
    at, out = ctp & 0x3FFFFFFF, set()
    for r in range(cnt):
        if r < pivot:
            p = body[at] | (body[at + 1] << 8)
            at += 2
            if p & 0x8000:
                out.add(p >> 12)
        else:
            p = body[at] | (body[at + 1] << 8) | (body[at + 2] << 16)
            at += 3
            if p & 0x800000:
                out.add(p >> 19)
    return out


def _cases(F, longest):
    """[(name, body, ctp, count, pivot, n_comp)] for F indexed fields"""
    rng = np.random.default_rng(1000 * F + longest)
    other = [f for f in range(F) if f != longest]
    out = []

    def add(name, docs, postings, limit=32768, ngram_vecs=None, ctype=None):
        body, ctp, cnt, pivot = RF.encode_key_body_fields(docs, postings, F, longest, 0, limit, ngram_vecs)
        if ctype is not None:
            assert ctp >> 30 == ctype, (name, ctp >> 30)
        out.append((name, body, ctp, cnt, pivot, 1 if ngram_vecs is None else len(ngram_vecs[0])))
        return pivot

    def pos(tf, max_gap=40):
        return RF.random_positions(rng, tf, max_gap)

    def vec(fields, tfs):
        return [(f, pos(t, 6 if t > 1000 else 40)) for f, t in zip(fields, tfs)]

    def rand_posting():
        k = int(rng.integers(1, min(F, 3) + 1))
        fs = sorted(int(x) for x in rng.choice(F, k, replace=False))
        return vec(fs, [int(rng.integers(5, 12)) for _ in fs])  # (5 positions at least: never embedded)

    # ---- only the longest field: counts of 1, 2 and 3 bytes, behind 2-byte and 3-byte pointers
    only = [[(longest, pos(5))], [(longest, pos(63))], [(longest, pos(64))], [(longest, pos(300))], [(longest, pos(8191, 7))], [(longest, pos(9000, 7))]]
    add("only-longest counts", _spaced(len(only)), only, ctype=RF.CT_ARRAY)
    assert add("only-longest counts, 3-byte pointers", _spaced(len(only)), only, limit=0) == 0
    # ---- vectors of 2, 3 and F entries, tfs of every VINT size (1 byte: meta bits <= 6; 2 bytes: <= 13; 3 bytes)
    sizes = (2, 100, 5000)
    vecs = []
    for k in sorted({2, min(3, F), F}):
        fs = list(range(k)) if k == F else sorted(int(x) for x in rng.choice(F, k, replace=False))
        for shift in range(3):
            vecs.append(vec(fs, [sizes[(i + shift) % 3] for i in range(k)]))
    vecs.append(vec([other[0]], [5]))      # one field that is not the longest: the general form with one entry
    vecs.append(vec([other[-1]], [5000]))
    add("field vectors", _spaced(len(vecs)), vecs, ctype=RF.CT_ARRAY)
    add("field vectors, 3-byte pointers", _spaced(len(vecs)), vecs, limit=0)
    # ---- embedded pointers: every tag.  2 bytes: 0xC .. 0xF only the longest (1 / 2 positions, with and without the top data bit),
    # 0x8 .. 0xA one other field of 1 - 3 positions, 0xB two fields
    a, b = (other[0], other[1]) if len(other) > 1 else (min(other[0], longest), max(other[0], longest))
    emb2 = [[(longest, [3])], [(longest, [5000])], [(longest, [3, 5])], [(longest, [40, 50])],
            [(other[0], [1])], [(other[0], [1, 2])], [(other[0], [1, 3, 5])], [(a, [1]), (b, [2])]]
    add("embedded 2-byte tags", _spaced(len(emb2)), emb2, ctype=RF.CT_ARRAY)
    assert _tags(*out[-1][1:5]) == set(range(0x8, 0x10)), (F, sorted(_tags(*out[-1][1:5])))
    c3 = sorted([a, b, [f for f in range(F) if f not in (a, b)][0]]) if F > 2 else None
    emb3 = [[(longest, [3])], [(longest, [600000])], [(longest, [3, 5])], [(longest, [600, 700])], [(longest, [1, 3, 5])], [(longest, [40, 50, 60])],
            [(longest, [1, 3, 5, 7])], [(longest, [20, 22, 24, 26])],
            [(other[0], [9])], [(other[0], [9, 11])], [(other[0], [1, 3, 5])], [(other[0], [1, 3, 5, 7])],
            [(a, [1]), (b, [2])], [(a, [1]), (b, [2, 4])], [(a, [1, 3]), (b, [2])]]
    if c3:
        emb3.append([(c3[0], [1]), (c3[1], [2]), (c3[2], [3])])
    assert add("embedded 3-byte tags, pivot 0", _spaced(len(emb3)), emb3, limit=0) == 0
    want3 = set(range(0x10, 0x17)) | set(range(0x18, 0x20)) | ({0x17} if c3 else set())
    assert _tags(*out[-1][1:5]) == want3, (F, sorted(hex(t) for t in _tags(*out[-1][1:5])))
    # ---- the pivot
    recs = [rand_posting() for _ in range(40)]
    assert 0 < add("pivot in the middle", _spaced(40), recs, limit=120) < 40
    assert add("pivot at the count", _spaced(40), recs) == 40
    mixed = [emb3[i % len(emb3)] if i % 3 else rand_posting() for i in range(60)]
    assert 0 < add("pivot in the middle, embedded and recorded", _spaced(60), mixed, limit=100) < 60
    # ---- containers
    for n in (1, 63, 64, 65):
        add(f"array {n}", _spaced(n), [rand_posting() for _ in range(n)], ctype=RF.CT_ARRAY)
    add("rle runs, one ending at 65535", [5, 9] + list(range(100, 200)) + list(range(65400, 65536)), [emb2[i % 4] if i % 2 else rand_posting() for i in range(238)],
        ctype=RF.CT_RLE)
    bits = sorted({63, 64, 65535} | {int(x) for x in rng.choice(np.arange(0, 65535, 5), 4200, replace=False)})
    add("bitmap bits 63 64 65535", bits, [emb2[i % len(emb2)] if i % 16 else rand_posting() for i in range(len(bits))], ctype=RF.CT_BITMAP)
    # ---- n-gram keys: the components' vectors in front of the key's own, every form of vector among them
    for nc in (2, 3):
        n = 24
        docs = _spaced(n)
        postings = [rand_posting() for _ in range(n)]

        def comp_vec(i, c):
            kind = (i + c) % 3
            if kind == 0:
                return [(longest, [1, 70, 9000][(i // 3) % 3])]
            fs = sorted(int(x) for x in rng.choice(F, 2 if kind == 1 else F, replace=False))
            return [(f, [3, 200, 5000][(i + f) % 3]) for f in fs]
        nv = [[comp_vec(i, c) for c in range(nc)] for i in range(n)]
        add(f"ngram {nc} components", docs, postings, ngram_vecs=nv)
        add(f"ngram {nc} components, 3-byte pointers", docs, postings, limit=60, ngram_vecs=nv)
    return out


def _write_cases(path, lib, N):
    rng = np.random.default_rng(11)
    blk = N.RefBlock()
    n_cases = n_variants = n_decoded = 0
    with open(path, "wb") as f:
        f.write(struct.pack("<II", 0x46444252, 0))
        for F in FIELD_COUNTS:
            d16, first = np.zeros(65536, np.uint16), np.zeros(65537, np.uint32)
            f8, t16 = np.zeros(65536 * F, np.uint8), np.zeros(65536 * F, np.uint16)
            for longest in (0, F - 1):
                for name, body, ctp, cnt, pivot, n_comp in _cases(F, longest):
                    for comp in range(n_comp):
                        buf = np.frombuffer(body, np.uint8).copy()
                        blk.block_id, blk.compression_type_pointer, blk.posting_count_m1, blk.pointer_pivot_p_docid = 0, ctp, cnt - 1, pivot
                        blk.byte_array = buf.ctypes.data

                        def host(length):
                            blk.byte_array_len = length
                            out = (N.ptr(d16, N.u16p), N.ptr(first, N.u32p), N.ptr(f8, N.u8p), N.ptr(t16, N.u16p))
                            if n_comp == 1:
                                return lib.ss_ref_decode_block_fields(C.byref(blk), F, longest, *out)
                            return lib.ss_ref_decode_block_fields_ngram(C.byref(blk), F, longest, n_comp, comp, *out)

                        variants = []

                        def record(kind, a, b, rc):
                            rec = struct.pack("<IIIi", kind, a, b, rc)
                            if rc >= 0:
                                w = int(first[rc])
                                dense = np.zeros((rc, F), np.uint16)
                                dense[np.repeat(np.arange(rc), np.diff(first[:rc + 1].astype(np.int64))), f8[:w]] = t16[:w]
                                rec += d16[:rc].tobytes() + dense.tobytes()
                            variants.append(rec)

                        rc = host(len(buf))
                        assert rc == cnt, (F, longest, name, rc)  # the case itself decodes
                        record(0, 0, 0, rc)
                        for length in range(len(buf)):         # byte_array_len truncated at every length
                            record(1, length, 0, host(length))
                        flips = [(int(rng.integers(0, len(buf))), 1 << int(rng.integers(0, 8))) for _ in range(FLIPS)]
                        # ... and every bit where the structure lies: the records' start, around the first pointers, the container's tail
                        first_ptr = ctp & 0x3FFFFFFF
                        spots = set(range(min(16, len(buf)))) | set(range(max(0, first_ptr - 8), min(len(buf), first_ptr + 8))) | \
                            set(range(max(0, len(buf) - 24), len(buf)))
                        if cnt <= 100:  # small blocks: every bit of every record and pointer
                            spots |= set(range(min(len(buf), 400)))
                        flips += [(at, 1 << bit) for at in sorted(spots) for bit in range(8)]
                        for at, mask in flips:
                            buf[at] ^= mask
                            record(2, at, mask, host(len(buf)))
                            buf[at] ^= mask
                        f.write(struct.pack("<IIIIIIII", ctp, cnt, pivot, n_comp, comp, F, longest, len(buf)) + buf.tobytes() + struct.pack("<I", len(variants)))
                        f.write(b"".join(variants))
                        n_cases += 1
                        n_variants += len(variants)
                        n_decoded += sum(1 for v in variants if struct.unpack_from("<i", v, 12)[0] >= 0)
        f.seek(4)
        f.write(struct.pack("<I", n_cases))
    return n_cases, n_variants, n_decoded


def test_field_vector_decoder_matches_the_host_decoder_under_sanitizers(tmp_path):
    from seekstorm_amd import _native as N
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "ref_block_fields_check")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(ROOT, "tests", "ref_block_fields_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    cases = str(tmp_path / "cases.bin")
    n_cases, n_variants, n_decoded = _write_cases(cases, N.lib(), N)
    assert n_cases >= 8 * 25 and n_decoded > n_cases  # (some flipped copies still decode: their field vectors are compared too)
    r = subprocess.run([exe, cases], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and f"ref_block_fields ok: {n_cases} cases, {n_variants} variants" in r.stdout, r.stdout + r.stderr[-4000:]


def test_new_entries_check_their_arguments_and_are_declared():
    from seekstorm_amd import _native as N
    lib = N.lib()
    z64, z32 = C.c_uint64(), C.c_uint32()
    sizes = (C.byref(z64), C.byref(z64), C.byref(z64), C.byref(z32), C.byref(z32))
    nulls = (None,) * 10
    fake = C.c_void_p(1)  # (never dereferenced: the null argument is judged first)
    assert lib.ss_bm25_open_index_bin_levels_fields(None, None, None, 0) == N.SS_EINVAL
    assert lib.ss_bm25_open_index_bin_levels_fields(None, fake, None, 0) == N.SS_EINVAL
    assert lib.ss_bm25_open_index_bin_levels_fields(fake, None, None, 0) == N.SS_EINVAL
    assert lib.ss_bm25_level_read_fields(None, 0, 0, 0, *nulls, 0, 0, 0, 0, *sizes) == N.SS_EINVAL
    assert lib.ss_bm25_level_read_fields(fake, 0, 0, 0, *nulls, 0, 0, 0, 0, None, None, None, None, None) == N.SS_EINVAL
    hdr = open(os.path.join(ROOT, "include", "seekstorm_hip.h")).read()
    ffi = open(os.path.join(ROOT, "integration", "hip_ffi.rs")).read()
    for name in ("ss_bm25_open_index_bin_levels_fields", "ss_bm25_level_read_fields"):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert re.search(r"\bfn\s+%s\s*\(" % name, ffi), name
    assert int(re.search(r"#define\s+SS_ABI_VERSION\s+(\d+)", hdr).group(1)) == 7  # the change is additive
