"""CPU tier of the dispatch counters (sprintz_mi355x_dispatch_counts / _name, SPRINTZ_KF_*; include/sprintz_mi355x.h): the symbols, the
names against the header's constants, the capacity contract, and that a call which fails before its launch moves no counter.  What
the counters say about the kernels is the GPU tier's (tests/test_gpu_dispatch.py and the modules that use tests/dispatch.py)."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the header's numbers are part of the ABI (new families are appended): stated here once more, so that a renumbering shows up as a diff of this test
FAMILIES = ["dec_big", "dec_any", "dec_verbatim", "dec_lat", "dec_row", "dec_blk", "dec_fast", "dec_uni", "dec_generic",
            "gather_fast", "gather_generic",
            "enc_big", "enc_any", "enc_lat", "enc_blk", "enc_blk_uni", "enc_pair", "enc_fast", "enc_wide", "enc_split", "enc_uni", "enc_generic",
            "dense_fused", "dense_verbatim", "dense_compact",
            "tr_chain", "tr_wave", "tr_levels", "on_chain", "on_three", "huf0_big", "huf0_sync", "huf0_default"]


def header_constants():
    with open(os.path.join(ROOT, "include", "sprintz_mi355x.h")) as f:
        return {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define SPRINTZ_KF_(\w+) (\d+)\s*$", f.read(), flags=re.M)}


def test_both_symbols_are_exported_and_bound():
    from sprintz_amd import _lib
    for name in ("sprintz_mi355x_dispatch_counts", "sprintz_mi355x_dispatch_name"):
        assert name in _lib.EXPORTED_SYMBOLS
        assert getattr(_lib.lib, name) is not None
    assert _lib.abi_version() == 7                       # additive: the version does not move


def test_names_match_the_header_constants():
    from sprintz_amd import _lib
    consts = header_constants()
    n = consts.pop("COUNT")
    assert n == _lib.KF_COUNT == len(FAMILIES) == _lib._dispatch_counts(None, 0)
    assert sorted(consts.values()) == list(range(n))     # dense, no number twice
    names = [_lib._dispatch_name(k) for k in range(n)]
    assert all(names) and all(re.fullmatch(rb"[a-z0-9_]+", s) for s in names)
    names = [s.decode() for s in names]
    assert len(set(names)) == n
    assert names == FAMILIES == _lib.KF_NAMES
    for const, k in consts.items():                      # SPRINTZ_KF_DEC_ROW <-> "dec_row"
        assert names[k] == const.lower(), (const, k, names[k])
    assert [_lib._dispatch_name(k) for k in range(n)] == [s.encode() for s in names]     # stable from call to call


def test_names_out_of_range_are_null():
    from sprintz_amd import _lib
    for k in (-1, _lib.KF_COUNT, _lib.KF_COUNT + 1, 1 << 30, -(1 << 31)):
        assert _lib._dispatch_name(k) is None


@pytest.mark.parametrize("capacity", [0, 1, 5, 32])
def test_a_small_capacity_writes_only_that_many_words(capacity):
    from sprintz_amd import _lib
    n = _lib.KF_COUNT
    assert capacity < n
    guard = 0xA5A5A5A5A5A5A5A5
    buf = (C.c_uint64 * (n + 4))(*([guard] * (n + 4)))
    assert _lib._dispatch_counts(buf, capacity) == n
    assert all(v != guard for v in buf[:capacity]) and all(v == guard for v in buf[capacity:])
    assert list(buf[:capacity]) == list(_lib.dispatch_counts().values())[:capacity]


def test_capacity_above_the_count_and_negative():
    from sprintz_amd import _lib
    n = _lib.KF_COUNT
    guard = 0xA5A5A5A5A5A5A5A5
    buf = (C.c_uint64 * (n + 4))(*([guard] * (n + 4)))
    assert _lib._dispatch_counts(buf, n + 4) == n
    assert all(v == guard for v in buf[n:])
    buf2 = (C.c_uint64 * 2)(guard, guard)
    assert _lib._dispatch_counts(buf2, -3) == n and list(buf2) == [guard, guard]
    assert _lib._dispatch_counts(None, n) == n           # nowhere to write: the count alone
    d = _lib.dispatch_counts()
    assert list(d) == FAMILIES and all(isinstance(v, int) and v >= 0 for v in d.values())


def test_calls_that_fail_before_their_launch_move_no_counter():
    """SPRINTZ_E_INVALID everywhere; SPRINTZ_E_NO_DEVICE where there is no device (with one, valid-looking arguments would launch on these
    host addresses: not tried)"""
    import numpy as np
    import torch
    from sprintz_amd import _lib
    E = _lib
    buf = np.zeros(1 << 14, np.uint8)
    p = (buf.ctypes.data + 4095) & ~4095
    before = _lib.dispatch_counts()
    assert _lib.compress_batch(0, 2, p, 100, 0, 8, p, 1024, p, None, None) == E.E_INVALID                       # chunk_len == 0
    assert _lib.compress_batch(0, 2, p, 100, 50, 8, p + 8, 1024, p, None, None) == E.E_INVALID                  # misaligned slots
    assert _lib.compress_batch_dense(0, 2, p, 100, 50, 8, p, 1024, p, None, None, p, p, None) == E.E_INVALID     # no container
    assert _lib.compact(p, 1024, p, 1, 3, p, p, p, None) == E.E_INVALID                                          # align not a power of two
    assert _lib.decompress_batch(0, 2, None, p, 1, 50, 8, p, None, None) == E.E_INVALID
    assert _lib.decompress_batch(0, 3, p, p, 1, 50, 8, p, None, None) == E.E_INVALID                            # elem_bytes
    assert _lib.gather_rows(0, 2, p, p, 1, 50, 8, p, 1, 1, p, None, None) == E.E_INVALID                         # chunk_len % ndims
    assert _lib.transform_decode_device(0, 2, None, 10, 8, p, p, None) < 0
    assert _lib.online_unpack_device(0, p + 1, 100, p, None, p, None) == E.E_INVALID                             # misaligned source
    assert _lib.huf0_decompress_batch_hint(None, p, 1, p, p, None, p, 0, None) == E.E_INVALID
    if not torch.cuda.is_available():
        assert _lib.compress_batch(0, 2, p, 100, 50, 8, p, 1024, p, None, None) == E.E_NO_DEVICE
        assert _lib.compress_batch_dense(0, 1, p, 4096, 1024, 32, p, 2048, p, None, p, p, p, None) == E.E_NO_DEVICE
        assert _lib.compact(p, 1024, p, 1, 16, p, p, p, None) == E.E_NO_DEVICE
        assert _lib.decompress_batch(0, 1, p, p, 4, 1024, 32, p, None, None) == E.E_NO_DEVICE
        assert _lib.gather_rows(1, 2, p, p, 4, 64, 8, p, 1, 4, p, None, None) == E.E_NO_DEVICE
        assert _lib.query_batch(1, 2, p, p, 1, 50, 8, 1, 0, 0, None, p, None, None) == E.E_NO_DEVICE
        assert _lib.transform_decode_device(0, 2, p, 1024, 8, p, p, None) == E.E_NO_DEVICE
        assert _lib.online_unpack_device(0, p, 100, p, None, p, None) == E.E_NO_DEVICE
        assert _lib.huf0_decompress_batch_hint(p, p, 1, p, p, None, p, 0, None) == E.E_NO_DEVICE
    assert _lib.dispatch_counts() == before


def test_the_helper_reports_every_family_that_moved():
    """tests/dispatch.py's assertion, on made-up deltas (no device needed)"""
    import dispatch
    dispatch.check({"dec_row": 1, "enc_blk": 1}, {"dec_row": 1, "dec_fast": 0})
    dispatch.check({"dec_row": 1}, {"dec_row": 1}, only=["dec_row"])
    dispatch.check({"dec_fast": 2}, never=["dec_row", "dec_blk"])
    with pytest.raises(AssertionError, match=r"dec_row: 0 launches, expected 1.*every family that moved: \{'dec_fast': 1, 'enc_blk': 1\}"):
        dispatch.check({"dec_fast": 1, "enc_blk": 1}, {"dec_row": 1})
    with pytest.raises(AssertionError, match=r"dec_fast: 1 launches, expected 0"):
        dispatch.check({"dec_fast": 1, "dec_row": 1}, {"dec_row": 1, "dec_fast": 0})
    with pytest.raises(AssertionError, match=r"dec_blk: 1 launches, expected never"):
        dispatch.check({"dec_blk": 1}, never=["dec_blk"])
    with pytest.raises(AssertionError, match=r"dense_compact: 1 launches, expected only \['enc_blk'\]"):
        dispatch.check({"enc_blk": 1, "dense_compact": 1}, {"enc_blk": 1}, only=["enc_blk"])
    with pytest.raises(AssertionError, match="unknown kernel family 'dec_rows'"):
        dispatch.check({}, {"dec_rows": 1})
    before = dispatch.counts()
    with dispatch.ran(only=[]):                            # a body that launches nothing
        pass
    assert dispatch.moved(before, dispatch.counts()) == {}
