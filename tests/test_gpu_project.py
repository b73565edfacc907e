"""GPU tests (-m gpu) of project rows (sprintz_mi355x_project_rows, ChunkedCodec.project_rows): the columns a slot table names, decoded
straight into a dense [G, K] tensor, in the element type or as float rows convert.

The expected value is always the numpy model (tests/project_model.py) on the ORIGINAL input, compared exactly; expected floats are torch's
CPU expression on the sliced input, bit for bit (checked against the model's bits too).  Every launch runs on a sentinel-filled output and
rets with padding around them, and asserts its kernel family (tests/dispatch.py) against the planner's answer for the shape
(tests/plan_probe.cpp, asked with q=16 rows=K out_esz=...)."""
import ctypes as C
import zlib

import numpy as np
import pytest

import float_model as fm
import planner
import project_model as pm
from drive_tables import ROWOP_CASES, ROWOP_IDS, fire_batch, rowop_batch
from drive_tables import FIRE_SHAPES as FIRE_TABLE
from fixtures import chunks_per_group, no_fast, sz  # noqa: F401  (fixtures)
from rowdata import FLOAT_FAST_SHAPES as FAST_SHAPES, GENERIC_SHAPES, gen_data, lowdim, make_batch
from streams import OLD, options, truncated_batch
from dispatch import ran
from harness import DTYPES

pytestmark = pytest.mark.gpu

PAD = 1024                                             # sentinel elements in front of and behind the output
SENT = {1: 0x5A, 2: 0x5A5A, 4: 0x5A5A5A5A}
CODEC_ID = {"delta": 0, "xff": 1}
Q_PROJECT = 16
RAW = pm.RAW
FORMATS = (RAW,) + fm.FORMATS


@pytest.fixture(scope="module")
def plan():
    """the planner on a host compiler: -> f(**fields) -> the family's name"""
    planner.available(required=True)

    known = {}

    def ask(**fields):
        key = tuple(sorted((k, int(v)) for k, v in fields.items()))
        if key not in known:                               # (one probe process a distinct question)
            got = planner.ask("decode", q=Q_PROJECT, **fields)
            assert got.get("family") in ("dec_fast", "dec_generic"), got
            known[key] = got["family"]
        return known[key]
    return ask


def out_bytes(esz, fmt):
    return esz if fmt == RAW else fm.OUT_BYTES[fmt]


def params(K):
    """per-slot scale and offset: slot j takes pair j % 8 of float_model's, so that a value converted with another slot's shows"""
    return fm.column_params(K)


def torch_want(x, D, cols, fmt, scale, offset, signed):
    """torch's CPU expression on the sliced input -> bits [G, K]; the elements that do not exist hold whatever 0 converts to (not compared)"""
    import torch
    rows, _ = pm.padded(x, D)
    sel = np.ascontiguousarray(rows[:, cols])
    if fmt == RAW:
        return sel
    t = torch.from_numpy(sel.view({1: np.int8, 2: np.int16}[sel.dtype.itemsize]) if signed else sel.astype(np.int32))
    dt = {fm.F32: torch.float32, fm.F16: torch.float16, fm.BF16: torch.bfloat16}[fmt]
    z = (t.to(torch.float32) * torch.from_numpy(scale) + torch.from_numpy(offset)).to(dt)
    return z.view(torch.int32 if fmt == fm.F32 else torch.int16).numpy().view(fm.BITS_DTYPE[fmt])


def run_project(batch, codec, esz, D, chunk_len, table, K, fmt=RAW, scale=None, offset=None, signed=False, general=False, shift=0, n=None):
    """the C entry point on sentinel-filled buffers: the output has PAD + shift elements in front, nchunks x R x K of its own -- a chunk slot each
    chunk, of which the first G x K are the result -- and PAD behind; rets one entry behind.  table: the int32 slot table as it is handed over.
    -> (the whole output buffer as bits, rets [nchunks + 1])"""
    import torch
    from sprintz_amd import _lib
    nch = batch.nchunks
    n = batch.total_len if n is None else n
    G = -(-n // D)
    osz = out_bytes(esz, fmt)
    dt = {1: torch.int8, 2: torch.int16, 4: torch.int32}[osz]
    assert G <= nch * (chunk_len // D)
    buf = torch.full((PAD + shift + nch * (chunk_len // D) * K + PAD,), SENT[osz], dtype=dt, device="cuda")
    rets = torch.full((nch + 1,), -77, dtype=torch.int64, device="cuda")
    tab = torch.from_numpy(np.ascontiguousarray(table, np.int32)).cuda()
    sc = torch.from_numpy(scale).cuda() if scale is not None else None
    of = torch.from_numpy(offset).cuda() if offset is not None else None
    flags = (_lib.QUERY_GENERAL_LAYOUT if general else 0) | (_lib.FLOAT_SIGNED if signed else 0)
    _lib.check(_lib.project_rows(CODEC_ID[codec], esz, batch.data.data_ptr(), batch.offsets.data_ptr(), nch, chunk_len, D, tab.data_ptr(), K,
                                 0 if fmt == RAW else 1 + fmt, sc.data_ptr() if sc is not None else None, of.data_ptr() if of is not None else None, flags,
                                 buf.data_ptr() + (PAD + shift) * osz, rets.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    return buf.cpu().numpy().view({1: np.uint8, 2: np.uint16, 4: np.uint32}[osz]), rets.cpu().numpy()


def assert_project(buf, rets, x, chunk_len, nchunks, D, K, want, written, shift, msg, bad=()):
    """the output against `want` [G, K] wherever `written` says an element exists -- outside the chunks in `bad` -- and the sentinel everywhere else:
    in front, behind, and at the places of the last row's elements that do not exist; rets are the chunks' element counts, with the sentinel behind"""
    n = x.size
    G, R = -(-n // D), chunk_len // D
    sent = SENT[buf.dtype.itemsize]
    assert buf.size == PAD + shift + nchunks * R * K + PAD, (buf.size,) + msg
    assert np.all(buf[:PAD + shift] == sent), ("written in front",) + msg
    assert np.all(buf[PAD + shift + G * K:] == sent), ("written behind the batch's last row",) + msg
    body = buf[PAD + shift:PAD + shift + G * K].reshape(G, K)
    assert want.shape == (G, K) and want.dtype == body.dtype, (want.shape, want.dtype, body.dtype) + msg
    assert np.all(body[~written] == sent), ("an element that does not exist was written",) + msg
    keep = written.copy()
    for c in bad:
        keep[c * R:(c + 1) * R] = False
    ne = (body != want) & keep
    assert not ne.any(), (int(ne.sum()), "of", int(keep.sum()), "elements differ; first at", tuple(int(v) for v in np.argwhere(ne)[0])) + msg
    lens = [min(chunk_len, n - c * chunk_len) for c in range(nchunks)]
    assert all(rets[c] == lens[c] for c in range(nchunks) if c not in bad) and all(rets[c] < 0 for c in bad) and rets[nchunks] == -77, ("rets", rets.tolist()) + msg


def rotate(key, k):
    return zlib.crc32(key.encode()) % k


def named_chunk_len(D):
    """67 rows: four groups of 16 and a verbatim tail of 3 rows"""
    return D * (16 * 4 + 3)


def column_sets(esz, D):
    """[0]; [D - 1]; two ascending, non-adjacent; all reversed; the identity; an odd K, permuted; at 8 bits an even and an odd K"""
    sets = [[0], [D - 1], list(range(D - 1, -1, -1)), list(range(D))]
    if D >= 3:
        sets += [[0, D - 1], [D - 1, 0, D // 2]]
    if D >= 4:
        sets += [[1, D - 1]]
    if D >= 5:
        sets += [[D - 2, 1, D - 1, 0], [3, D - 1, 0, 2, 1]]
    if D >= 8:
        sets += [[6, 1, 4, 7, 2, 5]]                       # six columns: at 16 bits a row of 12 bytes, so the 16-byte pieces wrap rows
    seen, out = set(), []
    for s in sets:
        if tuple(s) not in seen:
            seen.add(tuple(s))
            out.append(s)
    return out


def check_case(plan, batch, codec, esz, D, chunk_len, nchunks, x, cols, fmt, signed, general, fam, cpg, shift=0, bad=()):
    """one launch of one column set in one format, on the planner's family; -> that family"""
    K = len(cols)
    scale, offset = params(K) if fmt != RAW else (None, None)
    want = pm.project(x, chunk_len, D, cols, fmt, scale, offset, signed)
    written = pm.written(x.size, D, cols)
    tw = torch_want(x, D, cols, fmt, scale, offset, signed)
    assert np.array_equal(tw[written], want[written]), "the model differs from torch's CPU expression"
    osz = out_bytes(esz, fmt)
    family = plan(esz=esz, D=D, chunk_len=chunk_len, nchunks=nchunks, codec=CODEC_ID[codec], rows=K, out_esz=osz, general=general, no_fast=fam,
                  chunks_per_group=cpg, out_lo=(shift * osz) % 16)
    assert family == ("dec_fast" if pm.fast_takes(esz, D, chunk_len, K, osz, general, fam, (shift * osz) % 16) else "dec_generic")
    with ran(only=[family], **{family: 1}):
        buf, rets = run_project(batch, codec, esz, D, chunk_len, pm.slots(cols, D), K, fmt, scale, offset, signed, general, shift)
    assert_project(buf, rets, x, chunk_len, nchunks, D, K, want, written, shift, (codec, esz, D, cols, fmt, signed, general, fam, cpg, shift, family), bad)
    return family


# ------------------------------------------------------------------ parity

@pytest.mark.parametrize("codec,esz,D", [(codec, esz, D) for codec in ("delta", "xff") for esz, D in FAST_SHAPES + GENERIC_SHAPES])
def test_project_rows_parity_named_shapes(sz, oracle, no_fast, chunks_per_group, plan, codec, esz, D):
    """the sixteen shapes named for the planner, both codecs, both families (NO_FAST), 1 and 3 chunks a lane group, with and without the general
    layout, every column set in every format -- signed on (2, 8) and (1, 16) -- with a last chunk of 5 rows or one that ends mid-row.  The
    identity's raw output equals decompress byte for byte.  67 rows: four groups and a verbatim tail of 3"""
    import torch
    key = f"proj{codec}{esz}{D}"
    rng = np.random.default_rng(zlib.crc32(key.encode()))
    chunk_len = named_chunk_len(D)
    nchunks = 3 + D % 3
    last = 5 * D if rotate(key, 2) or D == 1 else 37 * D + max(1, D // 2)
    n = (nchunks - 1) * chunk_len + last
    x = gen_data(("walk", "uniform", "constant")[rotate(key, 3)], rng, n, esz, D)
    batches = {False: make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)}
    batches[True] = make_batch(sz, oracle, codec, esz, D, chunk_len, x, True) if lowdim(esz, D) else batches[False]
    seen = set()
    view = torch.int8 if esz == 1 else torch.int16
    for general in (False, True):
        cd, batch = batches[general]
        # (the general layout is another stream for the low-dim shapes alone: for the others one leg shows that the flag changes nothing)
        legs = ((0, 1), (0, 3), (1, 1)) if not general else ((0, 1), (1, 1)) if lowdim(esz, D) else ((0, 1),)
        for fam, cpg in legs:
            no_fast(fam)
            chunks_per_group(cpg)
            for cols in column_sets(esz, D):
                for fmt in (FORMATS if (fam, cpg) == (0, 1) or len(cols) != D else (RAW, fm.F32)):
                    for signed in ((False, True) if fmt != RAW and (esz, D) in ((2, 8), (1, 16)) else (False,)):
                        seen.add(check_case(plan, batch, codec, esz, D, chunk_len, nchunks, x, cols, fmt, signed, general, fam, cpg))
        # the identity, raw: decompress' bytes
        no_fast(0)
        chunks_per_group(1)
        buf, _ = run_project(batch, codec, esz, D, chunk_len, np.arange(D, dtype=np.int32), D, general=general)
        flat = cd.decompress(batch).reshape(-1).view(view).cpu().numpy().view(DTYPES[esz]) if not general or not lowdim(esz, D) else x
        assert np.array_equal(buf[PAD:PAD + n], flat[:n]) and np.array_equal(flat[:n], x)
    assert ("dec_fast" in seen) == ((esz, D) in ((2, 8), (2, 16), (2, 24), (2, 64), (1, 16))) and "dec_generic" in seen
    chunks_per_group(1)


@pytest.mark.parametrize("codec,esz,D,R", [("xff", 2, 8, 80), ("delta", 2, 4, 80), ("xff", 1, 6, 80), ("delta", 1, 8, 80), ("xff", 1, 64, 72), ("delta", 2, 33, 80),
                                           ("xff", 2, 40, 72), ("delta", 1, 32, 67), ("xff", 2, 12, 72)])
def test_project_rows_on_every_fast_mapping(sz, oracle, chunks_per_group, plan, codec, esz, D, R):
    """decode_fast.h's one-column-a-lane mappings that the named shapes leave out -- 4 and 8 lanes a chunk at either width, partly filled groups of
    16 and 64 -- with chunk slots that are and are not whole 16-byte pieces in the output, walks with flat spans (run blocks and the run shortcut)"""
    rng = np.random.default_rng(R * D + esz)
    chunk_len, nchunks = D * R, 5
    n = nchunks * chunk_len - 9 * D - D // 2
    x = gen_data("walk", rng, n, esz, D)
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    seen = set()
    for cpg in (1, 3):
        chunks_per_group(cpg)
        for cols in column_sets(esz, D):
            for fmt in FORMATS:
                seen.add(check_case(plan, batch, codec, esz, D, chunk_len, nchunks, x, cols, fmt, False, False, 0, cpg))
    assert "dec_fast" in seen
    chunks_per_group(1)


# ------------------------------------------------------------------ the two drives

@pytest.mark.parametrize("codec,w,D,kind", ROWOP_CASES, ids=ROWOP_IDS)
def test_project_rows_over_runs(sz, oracle, no_fast, chunks_per_group, plan, codec, w, D, kind):
    """tests/rle_drive.py's batches: runs of 1 .. 16 blocks and maximal ones, at chunk starts and ending at the chunk's last block -- the run blocks'
    stores and the cursor's advance count the projected block; on the planner's family at 1 and 3 chunks a lane group and on the generic kernel"""
    cd, batch, data, chunk_len, _ = rowop_batch(sz, oracle, codec, w, D, kind)
    esz = w // 8
    with options(**OLD):
        for fam, cpgs in ((0, (1, 3)), (1, (1,))):
            no_fast(fam)
            for cpg in cpgs:
                chunks_per_group(cpg)
                for cols in ([D - 1], [1, D - 2], [5, 0, 3], list(range(D - 1, -1, -1))):
                    for fmt in (RAW, fm.F32, fm.BF16):
                        check_case(plan, batch, codec, esz, D, chunk_len, batch.nchunks, data, cols, fmt, False, False, fam, cpg)
    chunks_per_group(1)
    no_fast(0)


@pytest.mark.parametrize("w,D", list(FIRE_TABLE), ids=[f"u{w}x{D}" for w, D in FIRE_TABLE])
def test_project_rows_on_the_fire_drive(sz, oracle, chunks_per_group, plan, w, D):
    """tests/fire_drive.py's batches: FIRE counters through their int16 wrap, runs replayed at frozen extreme coefficients -- the columns that are
    not stored keep their predictors exact, or the selected ones would not be"""
    cd, batch, data, chunk_len, nchunks = fire_batch(sz, oracle, w, D)
    with options(**OLD):
        for cpg in (1, 3):
            chunks_per_group(cpg)
            for cols in ([0], [D - 1], list(range(D - 1, -1, -1)))[:3 if D > 1 else 1]:
                for fmt in (RAW, fm.F16):
                    check_case(plan, batch, "xff", w // 8, D, chunk_len, nchunks, data, cols, fmt, False, False, 0, cpg)
    chunks_per_group(1)


# ------------------------------------------------------------------ the edges of the buffers

@pytest.mark.parametrize("codec,esz,D", [("xff", 2, 8), ("delta", 1, 16), ("delta", 2, 5), ("xff", 1, 7)])
def test_project_rows_edges_of_the_buffers(sz, oracle, plan, codec, esz, D):
    """an output off the 16-byte grid by one element and by 16, a last chunk that ends mid-row: nothing is written outside the [G, K] body nor at
    the places of elements that do not exist, and d_rets keeps the sentinel behind it"""
    rng = np.random.default_rng(7 * D)
    chunk_len, nchunks = D * (16 * 5 + 11), 4
    n = (nchunks - 1) * chunk_len + D * 37 + max(1, D // 2)
    x = gen_data("walk", rng, n, esz, D)
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    for shift in (0, 1, 16):
        for cols in ([0], [D - 1], [D - 1, 2, 0, 3], list(range(D))):
            for fmt in FORMATS:
                check_case(plan, batch, codec, esz, D, chunk_len, nchunks, x, cols, fmt, False, False, 0, 1, shift)


def test_project_rows_no_chunks(sz):
    import torch
    from sprintz_amd import _lib
    out = torch.full((64,), 0x5A5A, dtype=torch.int16, device="cuda")
    tab = torch.tensor([0, -1, 1, -1, -1, -1, -1, -1], dtype=torch.int32, device="cuda")
    offs = torch.zeros(1, dtype=torch.int64, device="cuda")
    with ran(only=[]):
        assert _lib.project_rows(1, 2, out.data_ptr(), offs.data_ptr(), 0, 8 * 67, 8, tab.data_ptr(), 2, 0, None, None, 0, out.data_ptr(), None, None) == 0
    torch.cuda.synchronize()
    assert torch.all(out == 0x5A5A)


# ------------------------------------------------------------------ damage

@pytest.mark.parametrize("codec,esz,D", [("xff", 2, 8), ("delta", 1, 32), ("delta", 2, 12)])
def test_project_rows_damaged_chunk(sz, oracle, chunks_per_group, plan, codec, esz, D):
    """one truncated chunk in the middle: its rets entry is negative and every other chunk's is its count (decompress_batch's); its neighbours are
    exact; check=True names the chunk"""
    import torch
    rng = np.random.default_rng(3 * D)
    chunk_len, nchunks, cut = named_chunk_len(D), 7, 3
    n = nchunks * chunk_len - 5 * D
    x = gen_data("walk", rng, n, esz, D)
    cd, good = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    batch = truncated_batch(sz, good, cut)
    with options(**OLD):
        chunks_per_group(3)
        plain_rets = torch.full((nchunks,), -77, dtype=torch.int64, device="cuda")
        cd.decompress(batch, rets=plain_rets)
        plain_rets = plain_rets.cpu().numpy()
        assert plain_rets[cut] < 0 and np.all(np.delete(plain_rets, cut) > 0)
        for cols in ([1], [D - 1, 0], list(range(D))):
            for fmt in (RAW, fm.F32):
                K = len(cols)
                scale, offset = params(K) if fmt != RAW else (None, None)
                family = plan(esz=esz, D=D, chunk_len=chunk_len, nchunks=nchunks, codec=CODEC_ID[codec], rows=K, out_esz=out_bytes(esz, fmt), chunks_per_group=3)
                with ran(only=[family], **{family: 1}):
                    buf, rets = run_project(batch, codec, esz, D, chunk_len, pm.slots(cols, D), K, fmt, scale, offset)
                assert np.array_equal(rets[:nchunks], plain_rets), (rets.tolist(), plain_rets.tolist())
                assert_project(buf, rets, x, chunk_len, nchunks, D, K, pm.project(x, chunk_len, D, cols, fmt, scale, offset), pm.written(n, D, cols), 0,
                               (codec, esz, D, cols, fmt), bad=(cut,))
        with pytest.raises(sz.SprintzError, match=f"project_rows: chunk {cut} "):
            cd.project_rows(batch, [0, D - 1])
        got = cd.project_rows(batch, [0, D - 1], check=False)
        assert got.shape == (n // D, 2)
        cd.project_rows(good, [0, D - 1])                                          # undamaged: no error
    chunks_per_group(1)


# ------------------------------------------------------------------ the slot table

@pytest.mark.parametrize("codec,esz,D,K", [("xff", 2, 8, 3), ("delta", 1, 16, 4), ("delta", 2, 5, 2), ("xff", 2, 64, 5), ("xff", 1, 80, 3)])
@pytest.mark.parametrize("fam", [0, 1], ids=["planned", "generic"])
def test_project_rows_slot_table_is_never_trusted(sz, oracle, no_fast, plan, codec, esz, D, K, fam):
    """a table of -1 with K valid entries, one entry >= K (K itself, and a huge one) and one < -1: every entry outside 0 .. K - 1 reads as "not
    wanted", so nothing is written outside the [G, K] body -- the sentinels around it stay -- and the valid entries' slots are exact.  These are
    valid inputs to a kernel that is robust by construction: each lane compares its entry, unsigned, against K before it forms an address"""
    rng = np.random.default_rng(K * D)
    chunk_len, nchunks = named_chunk_len(D), 4
    n = nchunks * chunk_len - 5 * D
    x = gen_data("uniform", rng, n, esz, D)
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    no_fast(fam)
    perm = rng.permutation(D)
    cols = [int(c) for c in perm[:K]]
    rest = [int(c) for c in perm[K:]]
    for beyond, below in ((K, -2), (0x7fffffff, -(1 << 31)), (K + 1, -K - 1)):
        table = pm.slots(cols, D).astype(np.int64)
        table[rest[0]] = beyond
        if len(rest) > 1:
            table[rest[1]] = below
        for fmt in (RAW, fm.F32, fm.BF16):
            scale, offset = params(K) if fmt != RAW else (None, None)
            osz = out_bytes(esz, fmt)
            family = plan(esz=esz, D=D, chunk_len=chunk_len, nchunks=nchunks, codec=CODEC_ID[codec], rows=K, out_esz=osz, no_fast=fam)
            with ran(only=[family], **{family: 1}):
                buf, rets = run_project(batch, codec, esz, D, chunk_len, table.astype(np.int32), K, fmt, scale, offset)
            assert_project(buf, rets, x, chunk_len, nchunks, D, K, pm.project(x, chunk_len, D, cols, fmt, scale, offset), pm.written(n, D, cols), 0,
                           (codec, esz, D, cols, beyond, below, fmt, family))
    no_fast(0)


# ------------------------------------------------------------------ Python

@pytest.mark.parametrize("codec,esz,D", [("xff", 2, 8), ("delta", 1, 5)])
def test_project_rows_python(sz, oracle, plan, codec, esz, D):
    import torch
    rng = np.random.default_rng(11 * D)
    chunk_len = named_chunk_len(D)
    n = 4 * chunk_len + 20 * D + D // 2                                            # a partial last row
    x = gen_data("uniform", rng, n, esz, D)
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    G = -(-n // D)
    view = torch.int8 if esz == 1 else torch.int16
    for cols in ([0], [D - 1, 1], list(range(D)), [3, 0, D - 1]):
        K = len(cols)
        family = plan(esz=esz, D=D, chunk_len=chunk_len, nchunks=5, codec=CODEC_ID[codec], rows=K, out_esz=esz)
        with ran(only=[family], **{family: 1}):
            got = cd.project_rows(batch, cols)
        assert got.shape == (G, K) and got.dtype == cd.dtype and got.device.type == "cuda" and got.is_contiguous()
        assert np.array_equal(got.view(view).cpu().numpy().view(DTYPES[esz]), pm.project(x, chunk_len, D, cols))      # zeros where the last row ends
        assert torch.equal(cd.project_rows(batch, torch.tensor(cols), general_layout=True).view(view), got.view(view))
        scale, offset = params(K)
        for dtype, fmt in ((torch.float32, fm.F32), (torch.float16, fm.F16), (torch.bfloat16, fm.BF16)):
            for signed in (False, True):
                f = cd.project_rows(batch, cols, dtype=dtype, scale=scale.tolist(), offset=torch.from_numpy(offset), signed=signed)
                assert f.shape == (G, K) and f.dtype == dtype
                bits = f.view(torch.int32 if fmt == fm.F32 else torch.int16).cpu().numpy().view(fm.BITS_DTYPE[fmt])
                assert np.array_equal(bits, pm.project(x, chunk_len, D, cols, fmt, scale, offset, signed))
        assert np.array_equal(cd.project_rows(batch, cols, dtype=torch.float32).cpu().numpy(), pm.project(x, chunk_len, D, cols).astype(np.float32))
        # out=: written in place; too small, of the wrong dtype or not contiguous is refused
        slot = batch.nchunks * (chunk_len // D) * K
        out = torch.zeros(slot + 7, dtype=cd.dtype, device="cuda")
        res = cd.project_rows(batch, cols, out=out)
        assert res.data_ptr() == out.data_ptr() and res.shape == (G, K) and torch.equal(res.view(view), got.view(view))
        rets = torch.full((batch.nchunks,), -1, dtype=torch.int64, device="cuda")
        cd.project_rows(batch, cols, rets=rets)
        assert rets.tolist() == [min(chunk_len, n - c * chunk_len) for c in range(batch.nchunks)]
        for bad in (torch.zeros(slot - 1, dtype=cd.dtype, device="cuda"), torch.zeros(slot, dtype=torch.float32, device="cuda"),
                    torch.zeros(slot * 2, dtype=cd.dtype, device="cuda")[::2], torch.zeros(slot, dtype=cd.dtype), np.zeros(slot)):
            with pytest.raises(ValueError):
                cd.project_rows(batch, cols, out=bad)
        with pytest.raises(ValueError):
            cd.project_rows(batch, cols, dtype=torch.float32, out=out)
    for bad in ([], [0, 0], [D], [-1], [0.5]):
        with pytest.raises(ValueError):
            cd.project_rows(batch, bad)
    for kw in (dict(scale=2.0), dict(offset=1.0), dict(signed=True)):               # a float dtype alone takes them
        with pytest.raises(ValueError):
            cd.project_rows(batch, [0], **kw)
    with pytest.raises(ValueError):
        cd.project_rows(batch, [0, 1], dtype=torch.float32, scale=[1.0, 2.0, 3.0])    # K entries, not ndims
    with pytest.raises(ValueError):
        cd.project_rows(batch, [0], dtype=torch.float64)
    with pytest.raises(ValueError):
        sz.ChunkedCodec(codec, esz, D, chunk_len + 1, device="cuda:0").project_rows(batch, [0])      # chunk_len % ndims != 0
