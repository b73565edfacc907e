"""Which kernel family served a call: assertions on the library's dispatch counters (sprintz_mi355x_dispatch_counts, SPRINTZ_KF_*).

Every kernel family of the library writes the same bytes as every other, so a byte comparison cannot tell a test whether the
kernel it names ran at all: a launch site that falls through to an older kernel produces exactly the bytes the test expects.
`ran` closes that gap -- it reads the counters before and after its body and checks the difference:

    with ran(dec_row=1, dec_fast=0):            # exactly these deltas (the families not named may move)
        codec.decompress(batch)
    with ran(enc_blk=1, only=["enc_blk", "dense_compact"]):   # ... and nothing but the listed families moved at all
        codec.compress(t)
    with ran(never=["dec_row", "dec_blk"]):     # none of these moved
        ...
    with ran(one_of=OLD_DECODERS):              # one launch in all among these, whichever of them took it

The counters are per process and count launches, not kernels' completions: nothing here synchronises."""
from contextlib import contextmanager

ROUND6 = ("enc_blk", "enc_blk_uni", "dec_blk", "dec_row")      # the delta kernels of SPRINTZ_OPT_BLK_CHUNKS / SPRINTZ_OPT_BLK_KERNELS
DECODERS = ("dec_big", "dec_any", "dec_verbatim", "dec_lat", "dec_row", "dec_blk", "dec_fast", "dec_uni", "dec_generic")
OLD_DECODERS = ("dec_verbatim", "dec_fast", "dec_uni", "dec_generic")      # what a batch decodes on with SPRINTZ_OPT_LAT_CHUNKS and _BLK_CHUNKS at 0
OLD_ENCODERS = ("enc_pair", "enc_fast", "enc_wide", "enc_split", "enc_uni", "enc_generic")
ENCODERS = ("enc_big", "enc_any", "enc_lat", "enc_blk", "enc_blk_uni", "enc_pair", "enc_fast", "enc_wide", "enc_split", "enc_uni", "enc_generic")


def counts():
    from sprintz_amd import _lib
    return _lib.dispatch_counts()


def moved(before, after):
    """{family: delta} of every family whose counter moved"""
    return {k: after[k] - before[k] for k in after if after[k] != before[k]}


def check(delta, expect=None, never=(), only=None, what="", one_of=None):
    """the assertion of `ran` on a {family: delta} dict (a plain function: the CPU tier tests it without a device)"""
    from sprintz_amd import _lib
    expect = expect or {}
    for k in list(expect) + list(never) + list(only or ()) + list(one_of or ()):
        assert k in _lib.KF_NAMES, f"unknown kernel family {k!r} (families: {_lib.KF_NAMES})"
    wrong = [f"{k}: {delta.get(k, 0)} launches, expected {v}" for k, v in expect.items() if delta.get(k, 0) != v]
    wrong += [f"{k}: {delta[k]} launches, expected never" for k in never if delta.get(k, 0)]
    if only is not None:
        wrong += [f"{k}: {delta[k]} launches, expected only {sorted(only)}" for k in delta if k not in only]
    if one_of is not None and sum(delta.get(k, 0) for k in one_of) != 1:
        wrong.append(f"{sum(delta.get(k, 0) for k in one_of)} launches among {list(one_of)}, expected 1")
    assert not wrong, f"dispatch{' of ' + what if what else ''}: " + "; ".join(wrong) + f" -- every family that moved: {dict(sorted(delta.items()))}"


@contextmanager
def ran(never=(), only=None, what="", one_of=None, **expect):
    before = counts()
    yield
    check(moved(before, counts()), expect, never, only, what, one_of)
