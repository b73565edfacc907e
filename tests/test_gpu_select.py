"""GPU tests (-m gpu) of select rows (sprintz_mi355x_select_rows, ChunkedCodec.select_rows / where): stream compaction fused into the
decode, in decode_fast.h and decode_kernel.h.  The expected value is always tests/select_model.py applied to the ORIGINAL input --
decode is lossless and pinned elsewhere.  Every batch ends in a short last chunk of whole rows."""
import zlib

import numpy as np
import pytest

import filter_model as fm
import select_model as sm
from dispatch import ran
from harness import DTYPES
from fixtures import no_fast, sentinels, sz  # noqa: F401  (fixtures)
from rowdata import bound_sets, chunk_len_for, existing_rows, gen_data, make_batch, parity_cases, parity_masks, short_batch
from rowop_runners import check_select, run_select

pytestmark = pytest.mark.gpu

SENTINELS = (0x5A, 0xA5)        # (the byte, repeated over the element / the id)


@pytest.mark.parametrize("codec,esz,D,shape,data,general", [c for c in parity_cases() if chunk_len_for(c[3], c[2]) % c[2] == 0])
def test_select_rows_parity(sz, oracle, no_fast, codec, esz, D, shape, data, general):
    """the whole-row shapes of test_gpu_query_windows.py's matrix x both families x eleven masks: rows and ids equal the model"""
    rng = np.random.default_rng(zlib.crc32(f"select{codec}{esz}{D}{shape}{data}{general}".encode()))
    chunk_len = chunk_len_for(shape, D)
    nchunks = 5 + D % 4
    x = gen_data(data, rng, short_batch(nchunks, chunk_len, D), esz, D)
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, general)
    all_rows = existing_rows(x, chunk_len, D)
    for name, mask in parity_masks(rng, x, chunk_len, esz, D):
        cnt = sm.counts(mask, x.size, chunk_len, D)
        total = int(cnt.sum())
        for fam in (0, 1):
            no_fast(fam)
            msg = (codec, esz, D, shape, data, general, fam, name)
            rows, _ = check_select(x, batch, codec, esz, D, chunk_len, mask, sm.prefix_bases(cnt), total, total, msg, general=general)
            if name in ("all rows", "every bit"):          # the existing rows of decompress
                assert np.array_equal(rows, all_rows), msg
            elif name == "no row":
                assert total == 0
            elif name in ("row 0", "last row"):
                assert total == nchunks


@pytest.mark.parametrize("codec,esz,D,chunk_len,fam,family", [
    ("xff", 2, 8, 5120, 0, "dec_fast"),
    ("delta", 1, 80, 10240, 0, "dec_fast"),       # two columns a lane, five pieces a row
    ("delta", 2, 24, 24 * 200, 0, "dec_fast"),    # group not full
    ("delta", 2, 12, 12 * 400, 0, "dec_generic"),  # 24-byte rows
    ("delta", 1, 1, 1024, 0, "dec_generic"),
    ("xff", 1, 3, 3000, 0, "dec_generic"),
    ("delta", 2, 300, 9600, 0, "dec_generic"),    # more than 256 columns
    ("xff", 2, 8, 5120, 1, "dec_generic"),        # any shape under OPT_NO_FAST
])
def test_select_rows_which_kernel(sz, oracle, no_fast, codec, esz, D, chunk_len, fam, family):
    no_fast(fam)
    rng = np.random.default_rng(D + fam)
    x = gen_data("walk", rng, short_batch(6, chunk_len, D), esz, D)
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    sets, _ = bound_sets(x, chunk_len, esz, D)
    name, mode, lo, hi, _ = sets[0]
    mask, cnt = fm.filter_rows(x, chunk_len, D, lo, hi, mode)
    total = int(cnt.sum())
    assert 0 < total < x.size // D
    with ran(only=[family], **{family: 1}):
        check_select(x, batch, codec, esz, D, chunk_len, mask, sm.prefix_bases(cnt), total, total, (codec, esz, D, family))


@pytest.mark.parametrize("codec", ["delta", "xff"])
@pytest.mark.parametrize("esz", [1, 2])
@pytest.mark.parametrize("D", [8, 16])
def test_select_rows_long_runs(sz, oracle, no_fast, codec, esz, D):
    """test_filter_rows_long_runs' data -- flat spans of 3 200 rows, runs of 400 blocks -- under masks that skip the run, take three
    rows deep inside it, and take all of it; the same with 16 columns, whose rows are whole 16-byte pieces at both widths"""
    R = 4096
    chunk_len = D * R
    top = (1 << (8 * esz)) - 1
    rng = np.random.default_rng(esz)
    nchunks = 3
    rows = nchunks * R - 700
    steps = rng.integers(-3, 4, size=(rows, D))
    x = np.mod(np.cumsum(steps, axis=0) + rng.integers(0, top, size=(1, D)), top + 1)
    flat = rng.integers(2, top - 1, D)
    for c in range(nchunks):
        x[c * R + 500:c * R + 3700] = flat                 # (the last chunk's span is cut short by the batch's end)
    x = x.astype(DTYPES[esz]).ravel()
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    outside = rng.random((nchunks, R)) < 0.5
    outside[:, 490:3710] = False                           # (the run's blocks and the rows around them)
    kinds = {"zero over the run": outside.copy(), "three rows inside": outside.copy(), "the whole run": np.zeros((nchunks, R), bool)}
    kinds["three rows inside"][:, [2000, 2001, 2777]] = True
    kinds["the whole run"][:, 500:3700] = True
    for name, bits in kinds.items():
        mask = np.packbits(bits, axis=1, bitorder="little")
        cnt = sm.counts(mask, x.size, chunk_len, D)
        total = int(cnt.sum())
        for fam, family in ((0, "dec_fast" if (D * esz) % 16 == 0 else "dec_generic"), (1, "dec_generic")):
            no_fast(fam)
            with ran(only=[family], **{family: 1}):
                got, _ = check_select(x, batch, codec, esz, D, chunk_len, mask, sm.prefix_bases(cnt), total, total, (codec, esz, D, fam, name))
            if name == "the whole run":
                assert np.all(got[:3200] == flat.astype(DTYPES[esz]))


LAYOUT_SHAPES = [
    ("xff", 2, 8, 5120),          # decode_fast
    ("delta", 1, 80, 10240),      # decode_fast, two columns a lane
    ("delta", 2, 12, 12 * 400),   # decode_kernel
    ("xff", 1, 3, 3000),          # decode_kernel, low-dimension layout
]


@pytest.mark.parametrize("codec,esz,D,chunk_len", LAYOUT_SHAPES)
def test_select_rows_bases_that_are_no_prefix_sums(sz, oracle, codec, esz, D, chunk_len):
    """the chunks in reverse order, and with five rows between them: the gaps keep the sentinel"""
    rng = np.random.default_rng(chunk_len)
    x = gen_data("walk", rng, short_batch(7, chunk_len, D), esz, D)
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    R, MB = fm.geometry(chunk_len, D)
    mask = np.packbits(rng.random((batch.nchunks, MB * 8)) < 0.3, axis=1, bitorder="little")
    cnt = sm.counts(mask, x.size, chunk_len, D)
    total = int(cnt.sum())
    reverse = sm.prefix_bases(cnt[::-1])[::-1]
    check_select(x, batch, codec, esz, D, chunk_len, mask, reverse, total, total, (codec, D, "reverse"))
    gaps = sm.prefix_bases(cnt + 5)
    out_rows = total + 5 * batch.nchunks
    want, want_ids = check_select(x, batch, codec, esz, D, chunk_len, mask, gaps, out_rows, out_rows, (codec, D, "gaps"))
    elem, ident = sentinels(esz, 0x5A)
    assert np.all(want[int(gaps[1]) - 5:int(gaps[1])] == elem) and np.all(want_ids[int(gaps[1]) - 5:int(gaps[1])] == ident)


@pytest.mark.parametrize("codec,esz,D,chunk_len,family", [
    ("xff", 2, 8, 5120, "dec_fast"),
    ("delta", 1, 80, 10240, "dec_fast"),
    ("delta", 2, 12, 12 * 400, "dec_generic"),
    ("delta", 1, 1, 1024, "dec_generic"),
])
def test_select_rows_output_guards(sz, oracle, codec, esz, D, chunk_len, family):
    """two sentinels, padded outputs: nothing past the total, nothing from a capacity's cut on, a NULL d_ids leaves the ids alone, and
    an output at an odd element offset takes the generic kernel and is still exact"""
    rng = np.random.default_rng(D)
    x = gen_data("walk", rng, short_batch(7, chunk_len, D), esz, D)
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    sets, _ = bound_sets(x, chunk_len, esz, D)
    R, MB = fm.geometry(chunk_len, D)
    masks = [fm.filter_rows(x, chunk_len, D, lo, hi, mode)[0] for _, mode, lo, hi, _ in sets[:2]]
    masks.append(np.full((batch.nchunks, MB), 0xFF, np.uint8))
    for j, mask in enumerate(masks):
        cnt = sm.counts(mask, x.size, chunk_len, D)
        total = int(cnt.sum())
        bases = sm.prefix_bases(cnt)
        for byte in SENTINELS:
            msg = (codec, D, j, byte)
            with ran(only=[family], **{family: 3}):
                check_select(x, batch, codec, esz, D, chunk_len, mask, bases, total, total, msg + ("total",), byte)
                check_select(x, batch, codec, esz, D, chunk_len, mask, bases, total // 2, total, msg + ("capacity",), byte)
                check_select(x, batch, codec, esz, D, chunk_len, mask, bases, total, total, msg + ("no ids",), byte, ids=False)
            with ran(only=["dec_generic"], dec_generic=1):
                check_select(x, batch, codec, esz, D, chunk_len, mask, bases, total, total, msg + ("odd offset",), byte, shift=1)


@pytest.mark.parametrize("codec,esz,D,chunk_len,fam", [
    ("xff", 2, 8, 5120, 0),       # decode_fast
    ("delta", 1, 80, 10240, 0),   # decode_fast, two columns a lane
    ("xff", 2, 8, 5120, 1),       # decode_kernel (NO_FAST)
    ("delta", 1, 1, 1024, 0),     # decode_kernel, low-dimension layout
])
def test_select_rows_damaged_chunk(sz, oracle, no_fast, codec, esz, D, chunk_len, fam):
    import torch
    no_fast(fam)
    rng = np.random.default_rng(5)
    nchunks = 9
    x = gen_data("walk", rng, short_batch(nchunks, chunk_len, D), esz, D)
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    bad = 4
    off = int(batch.offsets[bad].item())
    hdr = batch.data[off + 6:off + 8].clone()
    R, MB = fm.geometry(chunk_len, D)
    mask = np.packbits(rng.random((nchunks, MB * 8)) < 0.4, axis=1, bitorder="little")
    cnt = sm.counts(mask, x.size, chunk_len, D)
    total = int(cnt.sum())
    bases = sm.prefix_bases(cnt)
    elem, ident = sentinels(esz, 0x5A)
    want_rows, want_ids = sm.select_rows(x, chunk_len, D, mask, bases, total, sentinel=elem, id_sentinel=ident)
    batch.data[off + 6] = hdr[0] ^ 0x5                  # the header's ndims field
    rows, ids, rets = run_select(batch, codec, esz, D, chunk_len, mask, bases, total, total)
    assert rets[bad] < 0
    assert all(rets[c] == fm.chunk_counts(x.size, chunk_len)[c] for c in range(nchunks) if c != bad)
    keep = np.ones(total, bool)
    keep[int(bases[bad]):int(bases[bad] + cnt[bad])] = False       # the damaged chunk's span alone is unspecified
    assert np.all(rows[total * D:] == elem) and np.all(ids[total:] == ident)
    assert np.array_equal(rows[:total * D].reshape(total, D)[keep], want_rows[keep])
    assert np.array_equal(ids[:total][keep], want_ids[keep])
    mask_t, cnt_t = torch.from_numpy(mask).cuda(), torch.from_numpy(cnt).cuda()
    with pytest.raises(sz.SprintzError, match=f"chunk {bad} "):
        cd.select_rows(batch, mask_t, cnt_t, check=True)
    cd.select_rows(batch, mask_t, cnt_t, check=False)              # no error without the check
    batch.data[off + 6] = hdr[0]
    got = cd.select_rows(batch, mask_t, cnt_t, ids=True)           # repaired: no error, and exact
    assert np.array_equal(got["rows"].cpu().numpy().view(DTYPES[esz]), want_rows) and np.array_equal(got["ids"].cpu().numpy(), want_ids)


def test_select_rows_python(sz, oracle):
    import torch
    codec, esz, D, chunk_len = "xff", 2, 8, 5120
    rng = np.random.default_rng(21)
    x = gen_data("walk", rng, short_batch(6, chunk_len, D), esz, D)
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    sets, _ = bound_sets(x, chunk_len, esz, D)
    name, mode, lo, hi, _ = sets[0]                        # the band
    rows = x.reshape(-1, D)
    ok = ((rows >= lo) & (rows <= hi)).all(axis=1)
    assert 0 < ok.sum() < ok.size
    with ran(only=["dec_fast"], dec_fast=2):               # the filter launch and the select launch
        got = cd.where(batch, list(map(int, lo)), list(map(int, hi)), ids=True)
    assert got["rows"].dtype == cd.dtype and got["rows"].shape == (int(ok.sum()), D) and got["ids"].dtype == torch.int64
    assert np.array_equal(got["rows"].cpu().numpy().view(DTYPES[esz]), rows[ok])
    assert np.array_equal(got["ids"].cpu().numpy(), np.flatnonzero(ok))
    assert "ids" not in cd.where(batch, list(map(int, lo)), list(map(int, hi)))
    f = cd.filter_rows(batch, list(map(int, lo)), list(map(int, hi)))
    with_counts = cd.select_rows(batch, f["mask"], f["counts"], ids=True)
    without = cd.select_rows(batch, f["mask"], ids=True)
    assert torch.equal(with_counts["rows"].view(torch.int16), without["rows"].view(torch.int16)) and torch.equal(with_counts["ids"], without["ids"])
    assert np.array_equal(without["rows"].cpu().numpy().view(DTYPES[esz]), rows[ok])
    out = torch.zeros(rows.size, dtype=torch.int16, device="cuda:0").view(cd.dtype)
    into = cd.select_rows(batch, f["mask"], f["counts"], out=out)
    assert into["rows"].data_ptr() == out.data_ptr() and np.array_equal(into["rows"].cpu().numpy().view(DTYPES[esz]), rows[ok])
    none = cd.where(batch, 1, 0)                           # an empty interval: no row
    assert none["rows"].shape == (0, D)
    with pytest.raises(ValueError):
        cd.select_rows(batch, f["mask"][:, :-1])
    ragged = sz.ChunkedCodec("delta", 1, 80, 1024, device="cuda:0")        # 1 024 elements are no whole rows of 80
    rb = ragged.compress(torch.randint(0, 255, (1024 * 4,), dtype=torch.uint8, device="cuda:0"))
    with pytest.raises(ValueError):
        ragged.select_rows(rb, torch.zeros((4, 2), dtype=torch.uint8, device="cuda:0"))
    with pytest.raises(ValueError):
        ragged.where(rb, 0, 100)


def test_where_bench_size(sz):
    """the bench's headline input at full size, once: where() against torch's boolean index of the device-decoded batch"""
    import torch
    from rowdata import bench_input
    (codec, esz, D, chunk_len, nchunks), x = bench_input("cfg2", "cuda:0")
    cd = sz.ChunkedCodec(codec, esz, D, chunk_len, device="cuda:0")
    batch = cd.compress(x)
    dec = cd.decompress(batch).view(-1, D)
    top = (1 << (8 * esz)) - 1
    lo, hi = [0] * D, [top] * D
    for d in (0, D - 1):
        col = dec[:, d].to(torch.int32)
        nn = col.numel()
        lo[d] = int(torch.kthvalue(col, int(0.25 * (nn - 1)) + 1).values.item())     # the lower quantiles
        hi[d] = int(torch.kthvalue(col, int(0.75 * (nn - 1)) + 1).values.item())
        del col
    with ran(dec_fast=2):                                  # the filter launch and the select launch
        got = cd.where(batch, lo, hi, mode="all", ids=True)
    ok = torch.ones(dec.shape[0], dtype=torch.bool, device="cuda:0")
    for d in (0, D - 1):
        col = dec[:, d].to(torch.int32)
        ok &= (col >= lo[d]) & (col <= hi[d])
        del col
    total = int(ok.sum().item())
    assert 0 < total < ok.numel()
    want_ids = ok.nonzero().view(-1)
    assert got["rows"].shape == (total, D)
    assert torch.equal(got["ids"], want_ids)
    view = torch.int16 if esz == 2 else torch.int8
    assert torch.equal(got["rows"].view(view), dec.view(view)[want_ids])
