"""The per-posting block decoder that the host and the device decode kernels share (seekstorm_amd/csrc/ref_block_decode.h) on the CPU:
a stand-alone program (tests/ref_block_decode_check.cpp, its own main) is compiled with g++ under AddressSanitizer and UBSan and decodes
every case RANK BY RANK; the expected postings -- or the expected refusal -- of every case are what the library's whole-block host
decoder (ss_ref_decode_block / _ngram) answers for the same bytes.

Cases: every container (Array of 1, 2, 63, 64, 65, 4095 postings; Rle of one run, with single-doc runs, with a run ending at doc 65 535,
the full level of 65 536 postings whose last pointer is 3-byte; Bitmap of 4096 even docs and one with bits 63, 64, 65 535), every
embedded pointer tag of both sizes, the pivot at 0 / in the middle / at the count, tf VINTs of 1 - 3 bytes, n-gram bodies of 2 and 3
components (every component).  Corrupted copies (CPU only): byte_array_len truncated at EVERY length, single bytes flipped by a seeded
generator -- each must end in the host decoder's answer for those bytes, and in no sanitizer report (the bytes behind byte_array_len
are poisoned while a copy is decoded)."""
import ctypes as C
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from oracle import ref_format as RF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLIPS = 32  # seeded single-byte flips per case


def _spaced(n, step=3, first=1):
    return [first + step * i for i in range(n)]


def _cases():
    """[(name, body, ctp, count, pivot, n_comp)]"""
    rng = np.random.default_rng(20260)
    out = []

    def add(name, docs, positions, limit=32768, ngram_tfs=None, ctype=None):
        body, ctp, cnt, pivot = RF.encode_key_body(docs, positions, 0, limit, ngram_tfs)
        if ctype is not None:
            assert ctp >> 30 == ctype, (name, ctp >> 30)
        out.append((name, body, ctp, cnt, pivot, 1 if ngram_tfs is None else len(ngram_tfs[0])))
        return pivot

    def rand_pos(n, tf_hi=6):
        return [RF.random_positions(rng, int(rng.integers(1, tf_hi + 1))) for _ in range(n)]

    # ---- containers
    for n in (1, 2, 63, 64, 65, 4095):
        add(f"array {n}", _spaced(n, 3 if n < 4095 else 16), rand_pos(n), ctype=RF.CT_ARRAY)
    add("rle one run", list(range(100, 200)), rand_pos(100), ctype=RF.CT_RLE)
    add("rle single-doc runs", [5, 9, 13] + list(range(100, 200)) + [300, 65000], rand_pos(105), ctype=RF.CT_RLE)
    add("rle run ending at 65535", [7] + list(range(65000, 65536)), rand_pos(537), ctype=RF.CT_RLE)
    pivot = add("rle full level", list(range(65536)), [[1 + (i & 3)] for i in range(65536)], ctype=RF.CT_RLE)
    assert out[-1][3] == 65536 and pivot == 65535  # posting_count_m1 = 65535, the last posting's pointer is 3-byte
    add("bitmap 4096 even docs", list(range(0, 8192, 2)), rand_pos(4096, 3), ctype=RF.CT_BITMAP)
    bits = sorted({63, 64, 65535} | {int(x) for x in rng.choice(np.arange(0, 65535, 5), 4200, replace=False)})
    add("bitmap bits 63 64 65535", bits, rand_pos(len(bits), 3), ctype=RF.CT_BITMAP)
    # ---- pointers and tfs
    emb = [[3], [3, 5], [1, 3, 5], [1, 3, 5, 7], [9], [2, 9]]
    add("embedded 2-byte tags", _spaced(4), [[3], [3, 5], [100], [7, 9]], ctype=RF.CT_ARRAY)
    body, ctp = out[-1][1], out[-1][2]  # (no records: the pointers stand at the pointer range) tags 10 / 11 = one / two positions
    assert ctp & 0x3FFFFFFF == 0 and [body[2 * i + 1] >> 6 for i in range(4)] == [0b10, 0b11, 0b10, 0b11]
    assert add("embedded 3-byte tags, pivot 0", _spaced(len(emb)), emb, limit=0) == 0
    body, ctp = out[-1][1], out[-1][2]  # tags 100 .. 111 = one .. four positions
    assert ctp & 0x3FFFFFFF == 0 and [body[3 * i + 2] >> 5 for i in range(len(emb))] == [0b100, 0b101, 0b110, 0b111, 0b100, 0b101]
    recs = [RF.random_positions(rng, 5 + i % 4) for i in range(40)]
    pivot = add("pivot in the middle", _spaced(40), recs, limit=64)
    assert 0 < pivot < 40
    assert add("pivot at the count", _spaced(40), recs) == 40
    mixed = [emb[i % 4] if i % 3 else RF.random_positions(rng, 6) for i in range(60)]
    pivot = add("pivot in the middle, embedded and recorded", _spaced(60), mixed, limit=48)
    assert 0 < pivot < 60
    big = [list(range(0, 5)), list(range(0, 400, 2)), list(range(0, 60000, 3)), [4]]
    add("tf vints of 1, 2 and 3 bytes", _spaced(4), big)
    add("tf vints behind 3-byte pointers", _spaced(4), big, limit=0)
    # ---- n-gram keys: component tfs of every VINT size in front of the count
    for nc in (2, 3):
        n = 30
        ctf = np.stack([rng.choice([1, 2, 90, 300, 17000], n) for _ in range(nc)], axis=1)
        add(f"ngram {nc} components", _spaced(n), rand_pos(n), ngram_tfs=ctf)
        add(f"ngram {nc} components, 3-byte pointers", _spaced(n), rand_pos(n), limit=40, ngram_tfs=ctf)
    return out


def _write_cases(path, lib, N):
    d16, t16 = np.zeros(65536, np.uint16), np.zeros(65536, np.uint16)
    rng = np.random.default_rng(7)
    blk = N.RefBlock()
    n_cases = n_variants = n_decoded = 0
    with open(path, "wb") as f:
        f.write(struct.pack("<II", 0x31444252, 0))
        for name, body, ctp, cnt, pivot, n_comp in _cases():
            for comp in range(n_comp):
                buf = np.frombuffer(body, np.uint8).copy()
                blk.block_id, blk.compression_type_pointer, blk.posting_count_m1, blk.pointer_pivot_p_docid = 0, ctp, cnt - 1, pivot
                blk.byte_array = buf.ctypes.data

                def host(length):
                    blk.byte_array_len = length
                    if n_comp == 1:
                        return lib.ss_ref_decode_block(C.byref(blk), N.ptr(d16, N.u16p), N.ptr(t16, N.u16p))
                    return lib.ss_ref_decode_block_ngram(C.byref(blk), n_comp, comp, N.ptr(d16, N.u16p), N.ptr(t16, N.u16p))

                variants = []

                def record(kind, a, b, rc):
                    variants.append(struct.pack("<IIIi", kind, a, b, rc) + (d16[:rc].tobytes() + t16[:rc].tobytes() if rc >= 0 else b""))

                rc = host(len(buf))
                assert rc == cnt, (name, rc)  # the case itself decodes
                record(0, 0, 0, rc)
                top = int(d16[:cnt].max())
                record(3, top + 1, 0, rc)              # a level of exactly that many docs holds the block ...
                record(3, top, 0, N.SS_EINVAL)         # ... one doc fewer does not
                for length in range(len(buf)):         # byte_array_len truncated at every length
                    record(1, length, 0, host(length))
                flips = [(int(rng.integers(0, len(buf))), 1 << int(rng.integers(0, 8))) for _ in range(FLIPS)]
                if cnt <= 5000:  # ... and every bit where the structure lies: the records' start, around the first pointers, the container's tail
                    first_ptr = ctp & 0x3FFFFFFF
                    spots = set(range(min(16, len(buf)))) | set(range(max(0, first_ptr - 8), min(len(buf), first_ptr + 8))) | \
                        set(range(max(0, len(buf) - 40), len(buf)))
                    flips += [(at, 1 << bit) for at in sorted(spots) for bit in range(8)]
                for at, mask in flips:
                    buf[at] ^= mask
                    record(2, at, mask, host(len(buf)))
                    buf[at] ^= mask
                f.write(struct.pack("<IIIIII", ctp, cnt, pivot, n_comp, comp, len(buf)) + buf.tobytes() + struct.pack("<I", len(variants)))
                f.write(b"".join(variants))
                n_cases += 1
                n_variants += len(variants)
                n_decoded += sum(1 for v in variants if struct.unpack_from("<i", v, 12)[0] >= 0)
        f.seek(4)
        f.write(struct.pack("<I", n_cases))
    return n_cases, n_variants, n_decoded


def test_per_posting_decoder_matches_the_host_decoder_under_sanitizers(tmp_path):
    from seekstorm_amd import _native as N
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "ref_block_decode_check")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(ROOT, "tests", "ref_block_decode_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    cases = str(tmp_path / "cases.bin")
    n_cases, n_variants, n_decoded = _write_cases(cases, N.lib(), N)
    assert n_cases >= 25 and n_decoded > n_cases  # (some flipped copies still decode: their postings are compared too)
    r = subprocess.run([exe, cases], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and f"ref_block_decode ok: {n_cases} cases, {n_variants} variants" in r.stdout, r.stdout + r.stderr[-4000:]
