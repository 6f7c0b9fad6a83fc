"""The POSITIONS half of the per-posting block decoder that host and device share (seekstorm_amd/csrc/ref_block_decode.h: rbd_npos,
rbd_positions, the 64-bytes-at-a-time building block rbd_chunk_*) on the CPU: a stand-alone program
(tests/ref_block_positions_check.cpp, its own main) is compiled by the host compiler under AddressSanitizer and UBSan, run as a
subprocess, and walks every case RANK BY RANK in the host decoder's order; the expected counts and positions -- or the expected refusal
-- of every case are what the library's whole-block host decoder (ss_ref_decode_block_positions / _ngram_positions) answers for the same
bytes.  Every record that decodes is also decoded 64 bytes at a time, as a wave of the device takes it, and must give the same positions.

Cases: those of tests/test_ref_block_decode_cpu.py, plus stored position values at the 1 -> 2 -> 3-byte seams (127 / 128, 16383 / 16384),
a first position of 16384 and of 65535, a running position reaching exactly 65535 (accepted) and 65536 (SS_ENOTSUP), postings of 63, 64,
65 and 17000 positions, records whose 2- and 3-byte values straddle every offset of a 64-byte chunk boundary, n-gram records of 2 and 3
components with component tfs of every VINT size in front of the count.  Corrupted copies: byte_array_len truncated at EVERY length,
seeded single-byte flips, every bit around the record starts and the first pointers (the bytes behind byte_array_len are poisoned while
a copy is decoded)."""
import ctypes as C
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from oracle import ref_format as RF
from test_ref_block_decode_cpu import _cases as _container_cases, _spaced

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLIPS = 32  # seeded single-byte flips per case
POS_CAP = 1 << 21


def _from_stored(stored):
    """absolute positions of the stored values: the first as it is, then previous + stored + 1"""
    out = []
    for i, v in enumerate(stored):
        out.append(v if i == 0 else out[-1] + v + 1)
    return out


def _cases():
    """[(name, body, ctp, count, pivot, n_comp, expected code or None)]"""
    rng = np.random.default_rng(20261)
    out = [c + (None,) for c in _container_cases()]

    def add(name, positions, limit=32768, ngram_tfs=None, code=None):
        docs = _spaced(len(positions))
        body, ctp, cnt, pivot = RF.encode_key_body(docs, positions, 0, limit, ngram_tfs)
        out.append((name, body, ctp, cnt, pivot, 1 if ngram_tfs is None else len(ngram_tfs[0]), code))

    # ---- the seams of a stored value: 127 | 128 (one | two bytes), 16383 | 16384 (two | three), first and later values
    for v in (127, 128, 16383, 16384):
        for limit in (32768, 0):
            add(f"stored {v} first and later, pointers of {2 if limit else 3} bytes", [_from_stored([v, 1, v, 0, 2]), _from_stored([5, v, v])], limit)
    add("first position 16384", [[16384, 16390, 20000], [16384]])
    add("first position 65535", [[65535], [3, 65535], [65535]], limit=0)
    add("running position exactly 65535", [_from_stored([60000, 5000, 533]), [1, 2, 3]])
    assert _from_stored([60000, 5000, 533])[-1] == 65535
    add("running position 65536", [[1, 2, 3], _from_stored([60000, 5000, 534])], code=-4)
    # ---- long postings: one wave's bytes and one more, and many chunks (stored values of one byte, and of mixed sizes)
    for n in (63, 64, 65):
        add(f"{n} positions", [list(range(0, 3 * n, 3)), RF.random_positions(rng, n, 300), [7]])
    add("17000 positions", [[4], list(range(0, 51000, 3)), [1, 2]])
    mixed = _from_stored([int(x) for x in rng.choice([0, 1, 100, 127, 128, 129, 300], 170)] + [16384, 3, 16383, 0])
    assert mixed[-1] <= 65535
    add("170 positions of mixed sizes", [mixed, [9, 11]])
    # ---- a 2-byte and a 3-byte value at every offset across the boundary of a 64-byte chunk: lead one-byte values in front of them
    for lead in range(59, 67):
        add(f"chunk boundary, 3-byte value behind {lead} bytes", [_from_stored([1] * lead + [16384 + lead, 200, 2, 16500] + [3] * 70)])
        add(f"chunk boundary, 2-byte value behind {lead} bytes", [_from_stored([0] * lead + [128 + lead, 16384, 1] + [130] * 70), [2]])
    # ---- n-gram records: component tfs of every VINT size in front of the count, long and short position lists behind it
    for nc in (2, 3):
        n = 12
        ctf = np.stack([rng.choice([1, 127, 128, 16383, 16384, 65535], n) for _ in range(nc)], axis=1)
        pos = [RF.random_positions(rng, int(k)) for k in rng.choice([1, 2, 63, 64, 65, 130], n)]
        add(f"ngram {nc} components, positions", pos, ngram_tfs=ctf)
        add(f"ngram {nc} components, positions, 3-byte pointers", pos, limit=40, ngram_tfs=ctf)
    return out


def _write_cases(path, lib, N):
    d16, t16, n16 = np.zeros(65536, np.uint16), np.zeros(65536, np.uint16), np.zeros(65536, np.uint16)
    p16 = np.zeros(POS_CAP, np.uint16)
    n_pos = C.c_uint64()
    rng = np.random.default_rng(8)
    blk = N.RefBlock()
    n_cases = n_variants = n_decoded = 0
    with open(path, "wb") as f:
        f.write(struct.pack("<II", 0x32444252, 0))
        for name, body, ctp, cnt, pivot, n_comp, code in _cases():
            buf = np.frombuffer(body, np.uint8).copy()
            blk.block_id, blk.compression_type_pointer, blk.posting_count_m1, blk.pointer_pivot_p_docid = 0, ctp, cnt - 1, pivot
            blk.byte_array = buf.ctypes.data

            def host(length):
                blk.byte_array_len = length
                if n_comp == 1:
                    rc = lib.ss_ref_decode_block_positions(C.byref(blk), N.ptr(d16, N.u16p), N.ptr(t16, N.u16p), N.ptr(p16, N.u16p), POS_CAP, C.byref(n_pos))
                    if rc >= 0:
                        n16[:rc] = t16[:rc]
                    return rc
                return lib.ss_ref_decode_block_ngram_positions(C.byref(blk), n_comp, N.ptr(d16, N.u16p), N.ptr(t16, N.u16p), N.ptr(n16, N.u16p),
                                                               N.ptr(p16, N.u16p), POS_CAP, C.byref(n_pos))

            variants = []

            def record(kind, a, b, rc):
                v = struct.pack("<IIIi", kind, a, b, rc)
                if rc >= 0:
                    assert int(n_pos.value) <= POS_CAP
                    v += struct.pack("<I", int(n_pos.value)) + n16[:rc].tobytes() + p16[:int(n_pos.value)].tobytes()
                variants.append(v)

            rc = host(len(buf))
            assert rc == (cnt if code is None else code), (name, rc)  # the case itself decodes, or is refused as the case says
            record(0, 0, 0, rc)
            for length in range(len(buf)):  # byte_array_len truncated at every length
                record(1, length, 0, host(length))
            flips = [(int(rng.integers(0, len(buf))), 1 << int(rng.integers(0, 8))) for _ in range(FLIPS)]
            if cnt <= 5000:  # ... and every bit where the structure lies: the record starts, around the first pointers, the container's tail
                first_ptr = ctp & 0x3FFFFFFF
                spots = set(range(min(16, len(buf)))) | set(range(max(0, first_ptr - 8), min(len(buf), first_ptr + 8)))
                if len(buf) <= 4000:
                    spots |= set(range(max(0, len(buf) - 40), len(buf)))
                flips += [(at, 1 << bit) for at in sorted(spots) for bit in range(8)]
            for at, mask in flips:
                buf[at] ^= mask
                record(2, at, mask, host(len(buf)))
                buf[at] ^= mask
            f.write(struct.pack("<IIIII", ctp, cnt, pivot, n_comp, len(buf)) + buf.tobytes() + struct.pack("<I", len(variants)))
            f.write(b"".join(variants))
            n_cases += 1
            n_variants += len(variants)
            n_decoded += sum(1 for v in variants if struct.unpack_from("<i", v, 12)[0] >= 0)
        f.seek(4)
        f.write(struct.pack("<I", n_cases))
    return n_cases, n_variants, n_decoded


def test_per_posting_positions_match_the_host_decoder_under_sanitizers(tmp_path):
    from seekstorm_amd import _native as N
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "ref_block_positions_check")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(ROOT, "tests", "ref_block_positions_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    cases = str(tmp_path / "cases.bin")
    n_cases, n_variants, n_decoded = _write_cases(cases, N.lib(), N)
    assert n_cases >= 60 and n_decoded > n_cases  # (some flipped copies still decode: their positions are compared too)
    r = subprocess.run([exe, cases], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and f"ref_block_positions ok: {n_cases} cases, {n_variants} variants" in r.stdout, r.stdout + r.stderr[-4000:]
