"""The fixtures and small helpers that many test modules share.  A module takes a fixture by importing its name (under `# noqa: F401`);
pytest then sets it up once for that module."""
import ctypes as C
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sz():
    """the package, on a machine with a GPU"""
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import sprintz_amd
    return sprintz_amd


@pytest.fixture(scope="module")
def lib():
    """the ctypes binding, without a device; builds the library where a checkout has none yet"""
    if not os.path.exists(os.path.join(ROOT, "sprintz_amd", "libsprintz_mi355x.so")):
        import __graft_entry__
        __graft_entry__.build()
    from sprintz_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def gpu_lib():
    """the ctypes binding, on a machine with a GPU"""
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from sprintz_amd import _lib
    return _lib


@pytest.fixture
def no_fast():
    """set_option(OPT_NO_FAST) for the duration of a test, restored afterwards"""
    from sprintz_amd import _lib

    def setter(v):
        _lib.check(_lib.set_option(_lib.OPT_NO_FAST, int(v)))
    yield setter
    _lib.set_option(_lib.OPT_NO_FAST, 1 if os.environ.get("SPRINTZ_MI355X_NO_FAST") is not None else 0)


@pytest.fixture
def chunks_per_group():
    """set_option(OPT_CHUNKS_PER_GROUP) for the duration of a test, restored afterwards"""
    from sprintz_amd import _lib

    def setter(k):
        _lib.check(_lib.set_option(_lib.OPT_CHUNKS_PER_GROUP, int(k)))
    yield setter
    _lib.set_option(_lib.OPT_CHUNKS_PER_GROUP, int(os.environ.get("SPRINTZ_MI355X_CHUNKS_PER_GROUP", 1)))


def buf_fixture(size):
    """a module's `buf` fixture: (`size` bytes of host memory, an address in it on the 16-byte grid) for the validation tests' pointers"""
    @pytest.fixture(scope="module")
    def buf():
        b = (C.c_uint8 * size)()
        return b, (C.addressof(b) + 15) & ~15
    return buf


def refusals(lib, call, name=None):
    """-> (invalid, unsupported): call(**kw) must return E_INVALID / E_UNSUPPORTED and the message name the operation; without a name an
    E_INVALID must leave some message and an E_UNSUPPORTED is not asked for one"""
    def refused(code, needs_message, kw):
        got = call(**kw)
        assert got == code, ("returned", got, "for", code, kw)
        err = lib.last_error()
        if name is not None:
            assert name in err, ("the message does not name", name, kw, err)
        elif needs_message:
            assert err, ("no message", kw)
    return (lambda **kw: refused(lib.E_INVALID, True, kw)), (lambda **kw: refused(lib.E_UNSUPPORTED, False, kw))


def random_mask(rng, nchunks, MB, p):
    """a row mask of MB bytes a chunk, every bit set with probability p -- those of rows that do not exist too"""
    return np.packbits(rng.random((nchunks, MB * 8)) < p, axis=1, bitorder="little")


def sentinel(nbytes, byte):
    """`byte` repeated over an element of nbytes, as the integer a buffer filled with it reads as"""
    return int.from_bytes(bytes([byte]) * nbytes, "little")


def sentinels(esz, byte):
    """-> (`byte` over an element, `byte` over a signed 64-bit row id)"""
    return sentinel(esz, byte), int.from_bytes(bytes([byte]) * 8, "little", signed=True)
