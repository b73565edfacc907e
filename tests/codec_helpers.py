"""Helpers of the online coders', the Huffman stage's and the bit-packing primitives' tests, shared by their CPU and GPU tiers: the oracle's
online entry points and their golden streams (fixtures among them), the Huffman drive's per-case checks, and the known-answer streams' check."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import huf_drive as hd
import kat
from harness import ORACLE_SO


# ------------------------------------------------------------------ the online coders'

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden_online():
    gdir = os.path.join(ROOT, "tests", "golden")
    with open(os.path.join(gdir, "golden_online_v1.json")) as f:
        manifest = json.load(f)["cases"]
    return manifest, np.load(os.path.join(gdir, "golden_online_v1.npz"))


@pytest.fixture(scope="module")
def orc(oracle):
    lib = C.CDLL(ORACLE_SO)
    lib.online_oracle_pack.restype = C.c_int64
    lib.online_oracle_pack.argtypes = [C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(C.c_size_t)]
    lib.online_oracle_unpack.restype = C.c_int64
    lib.online_oracle_unpack.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
    lib.online_oracle_bound.restype = C.c_size_t
    lib.online_oracle_bound.argtypes = [C.c_int, C.c_uint32]
    return lib


def oracle_pack(lib, kind, x):
    x = np.ascontiguousarray(x, dtype=np.uint16)
    out = np.zeros(lib.online_oracle_bound(kind, x.size), np.uint8)
    nb = C.c_size_t(0)
    ret = lib.online_oracle_pack(kind, x.ctypes.data, x.size, out.ctypes.data, C.byref(nb))
    return out[: 2 * int(ret)].copy(), int(ret), int(nb.value)


def oracle_unpack(lib, kind, cont, n):
    buf = np.concatenate([np.ascontiguousarray(cont, dtype=np.uint8), np.zeros(64, np.uint8)])
    out = np.zeros(n + 16, np.uint16)
    ret = lib.online_oracle_unpack(kind, buf.ctypes.data, out.ctypes.data)
    return out[:n].copy(), int(ret)


# ------------------------------------------------------------------ the Huffman drive's

DECODE_CAP = 300_000             # symbols the Python bit reader may decode per test


def unpack(table):
    table = np.asarray(table, np.uint8)
    lens = np.zeros(256, np.uint8)
    lens[0::2], lens[1::2] = table & 15, table >> 4
    return lens


def check_case(case, chunk, huf, ho, tables, who="oracle"):
    """the record of a record case is on the side of its edge that the case claims: read from the record's own header, the fourth
    sub-stream's size (which no header field carries) from the drive's arithmetic and the record's length"""
    c = case["chunk"]
    rec = huf[int(ho[c]):int(ho[c + 1])]
    n, stored, sz = hd.record_header(rec)
    assert n == len(chunk), (who, case)
    if "n" in case:
        assert n == case["n"], (who, case)
        return
    assert stored == case["stored"], (who, case, n, stored, sz)
    own_stored, own = hd.record_sizes(chunk, unpack(tables[128 * (c // hd.SEG):128 * (c // hd.SEG) + 128]))
    assert own_stored == stored, (who, case)
    if "enc_minus_n" in case:
        assert sum(own) - n == case["enc_minus_n"], (who, case, own)
    if "sub" in case:
        assert own[case["sub"][0]] == case["sub"][1], (who, case, own)
    if stored:
        assert len(rec) == (4 + n + 3) & ~3 and bytes(rec[4:4 + n]) == chunk.tobytes(), (who, case)
    else:
        assert sz == own[:3] and len(rec) == (12 + sum(own) + 3) & ~3, (who, case, sz, own, len(rec))
        if case.get("sub", (0, 0))[0] == 3:
            assert own[3] >= 0xFFFF and max(sz) < 0xFFFF, (who, case, "only the sub-stream without a size field is long", own, sz)


def decode_sample(b, huf, ho, tables, who="oracle"):
    """decode_record of every edge record and of one record per segment (its largest chunk of at most 6 000 bytes; the largest of all
    where it has none), against the chunk; the long records only at the head of each of their sub-streams.  -> symbols decoded"""
    picks = [(c["chunk"], c.get("partial", False)) for c in b["cases"]]
    for sname, first in b["segments"]:
        sizes = [len(ch) for ch in b["chunks"][first:first + hd.SEG]]
        ok = [k for k, s in enumerate(sizes) if 0 < s <= 6000] or [int(np.argmax(sizes))]
        k = max(ok, key=lambda k: sizes[k])
        picks.append((first + k, sizes[k] > 6000))
    done = 0
    for c, partial in picks:
        chunk = b["chunks"][c]
        rec = huf[int(ho[c]):int(ho[c + 1])]
        tab = tables[128 * (c // hd.SEG):128 * (c // hd.SEG) + 128]
        if partial:
            got, mask = hd.decode_record(rec, tab, per_stream=1500)
            got = np.frombuffer(got, np.uint8)
            assert np.array_equal(got[mask], chunk[mask]), (who, c)
            done += int(mask.sum()) if not hd.record_header(rec)[1] else 0
        else:
            assert hd.decode_record(rec, tab) == chunk.tobytes(), (who, c)
            done += len(chunk)
    assert done <= DECODE_CAP, done
    return done


# ------------------------------------------------------------------ the bit-packing primitives'

# (width, columns, low-dim layout?)
KAT_SHAPES = [(8, 8, False), (8, 5, False), (8, 1, True), (8, 3, True), (8, 4, True),
          (16, 8, False), (16, 3, False), (16, 1, True), (16, 2, True)]


def check_kat_streams(streams, w, ndims, lowdim):
    """streams[e]: np.uint8 stream of chunk e (kat.kat_chunks); every header field, every payload byte, the run and the tail"""
    fields, nb, z = kat.expected_fields(w, ndims, lowdim)
    err = kat.kat_errors(w, ndims)
    hb = 3 if w == 8 else 4
    hdr = (2 * ndims * hb + 7) // 8
    esz = w // 8
    nblocks = kat.kat_rows(ndims) // 8
    # the delta codecs close a run when fewer than two blocks would remain (`<`, sprintz_delta_rle.cpp:226): blocks 1 .. nblocks - 3 are
    # the run, the last two blocks travel verbatim
    run, tail_rows = (1, 0) if nblocks == 2 else (nblocks - 3, 16)
    for e in range(1 << w):
        s = streams[e]
        if not fields[e].any():
            continue                                                 # (chunk 0 of a one-column shape: all zero, nothing of block 0 to read)
        assert int.from_bytes(bytes(s[0:4]), "little") == 1, (e, "one group")
        assert int(s[4]) | int(s[5]) << 8 == tail_rows * ndims and int(s[6]) | int(s[7]) << 8 == ndims, e
        got = kat.read_fields(s, w, ndims)
        assert np.array_equal(got[:ndims], fields[e]), (w, ndims, lowdim, e, got[:ndims], fields[e])
        assert not got[ndims:].any(), (e, "slot 1 is a run")
        payload = kat.expected_block_payload(z[e], nb[e], w, lowdim)
        at = 8 + hdr
        assert bytes(s[at:at + len(payload)]) == payload, (w, ndims, lowdim, e)
        at += len(payload)
        assert s[at] == run, (e, s[at], run)
        tail = np.tile(err[e], tail_rows).astype(np.uint8 if w == 8 else np.uint16).tobytes()
        assert bytes(s[at + 1:]) == tail, (w, ndims, lowdim, e)
