"""GPU tests (-m gpu) of zone-map pruning (sprintz_mi355x_zone_map / _zone_prune_box / _zone_prune_linear / _zone_expand, ChunkedCodec.zone_map
and the zones= argument of filter_rows / filter_linear / the *_where operations).  A call with zones must give bit for bit what the call
without gives; the expected value is always the filters' numpy models applied to the ORIGINAL input -- decode is lossless and pinned
elsewhere -- and the classes are tests/zone_model.py's.  Every comparison is exact.

The inputs are built so that all three classes occur: chunk c's values are level[c] + noise in 0 .. 15 with the levels cycling 0, 100,
110, 200, and the band is 90 .. 120 -- levels 0 and 200 lie outside it (NONE), 100 .. 115 inside (ALL), 110 .. 125 across its edge (DECODE)."""
import ctypes as C
import zlib

import numpy as np
import pytest

import filter_model as fm
import linear_model as lm
import zone_model as zm
from dispatch import DECODERS, ran
from harness import DTYPES
from fixtures import no_fast, sz  # noqa: F401  (fixtures)
from rowdata import gen_data, make_batch
from rowop_runners import assert_zone_map, host

pytestmark = pytest.mark.gpu

LEVELS = (0, 100, 110, 200)
BAND = (90, 120)


def level_data(rng, nchunks, chunk_len, esz, D, short=0, flat_last_column=False):
    """-> the flat input of nchunks chunks, the last one `short` elements short.  flat_last_column: the last column (of D > 1) stays at
    level 0 in every chunk, so that column 0 minus the last column follows the levels"""
    level = np.array(LEVELS, np.int64)[np.arange(nchunks) % 4].repeat(chunk_len)
    if flat_last_column and D > 1:
        level[np.arange(level.size) % chunk_len % D == D - 1] = 0
    x = level + rng.integers(0, 16, level.size)
    return x[:nchunks * chunk_len - short].astype(DTYPES[esz])


def stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def dev(a, dtype=None):
    """a numpy array -> a device tensor (uint16 through its signed twin: torch lacks most of uint16)"""
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        return torch.from_numpy(a.view(np.int16)).cuda().view(torch.uint16)
    t = torch.from_numpy(a).cuda()
    return t if dtype is None else t.to(dtype)


def box_bounds(esz, D, mode):
    """the band on every column under ALL; under ANY on the first and the last column, the others never matching"""
    top = (1 << (8 * esz)) - 1
    if mode == fm.ALL:
        return np.full(D, BAND[0], np.int64), np.full(D, BAND[1], np.int64)
    lo, hi = np.full(D, top, np.int64), np.zeros(D, np.int64)
    for d in (0, D - 1):
        lo[d], hi[d] = BAND
    return lo, hi


def raw_zoned(sz, cd, batch, codec, z, pred, outs="both", want_rets=True, sentinel=0x5A):
    """The C entry points themselves, in the documented order: prune, read n', the filter on the survivors into compact buffers, expand.
    pred: ("box", lo_t, hi_t, mode) or ("lin", w_t, bias, lo, hi).  Outputs are sentinel-filled and padded; -> dict of numpy arrays"""
    import torch
    from sprintz_amd import _lib
    n, D, esz, chunk_len = batch.nchunks, cd.ndims, cd.esz, cd.chunk_len
    R, MB = fm.geometry(chunk_len, D)
    cid = _lib.CODEC_DELTA if codec == "delta" else _lib.CODEC_XFF
    cls = torch.full((n + 8,), 0x77, dtype=torch.uint8, device="cuda")
    pos = torch.full((n + 1 + 4,), -0x1234, dtype=torch.int64, device="cuda")                # garbage beforehand: every entry must be overwritten
    surv = torch.full((n + 1 + 4,), -0x4321, dtype=torch.int64, device="cuda")
    tmp = torch.full((_lib.zone_prune_tmp_bytes(n) // 8,), -1, dtype=torch.int64, device="cuda")
    common = (esz, n, chunk_len, D, batch.offsets.data_ptr(), z.min.data_ptr(), z.max.data_ptr(), z.len.data_ptr())
    tail = (cls.data_ptr(), pos.data_ptr(), surv.data_ptr(), tmp.data_ptr(), stream())
    if pred[0] == "box":
        _lib.check(_lib.zone_prune_box(*common, pred[1].data_ptr(), pred[2].data_ptr(), pred[3], *tail))
    else:
        _lib.check(_lib.zone_prune_linear(*common, pred[1].data_ptr(), pred[2], pred[3], pred[4], *tail))
    ns = int(pos[n].item())
    ptr = lambda t: t.data_ptr() if t is not None else None      # noqa: E731
    cmask = torch.full((max(ns, 1) * MB,), 0x33, dtype=torch.uint8, device="cuda") if outs != "counts" else None
    ccounts = torch.full((max(ns, 1),), -9, dtype=torch.int32, device="cuda") if outs != "mask" else None
    crets = torch.full((max(ns, 1),), -99, dtype=torch.int64, device="cuda") if want_rets else None
    if ns:
        if pred[0] == "box":
            _lib.check(_lib.filter_rows(cid, esz, batch.data.data_ptr(), surv.data_ptr(), ns, chunk_len, D, pred[1].data_ptr(), pred[2].data_ptr(),
                                        pred[3], 0, ptr(cmask), ptr(ccounts), ptr(crets), stream()))
        else:
            _lib.check(_lib.filter_linear(cid, esz, batch.data.data_ptr(), surv.data_ptr(), ns, chunk_len, D, pred[1].data_ptr(), None, pred[2], pred[3],
                                          pred[4], 0, None, ptr(cmask), ptr(ccounts), ptr(crets), stream()))
    pad = 64
    mask = torch.full((1 + n * MB + pad,), sentinel, dtype=torch.uint8, device="cuda")       # the mask starts at an odd address
    counts = torch.full((n + pad,), -77, dtype=torch.int32, device="cuda")
    rets = torch.full((n + pad,), -7777, dtype=torch.int64, device="cuda")
    _lib.check(_lib.zone_expand(n, chunk_len, D, cls.data_ptr(), pos.data_ptr(), z.len.data_ptr(), ptr(cmask), ptr(ccounts), ptr(crets),
                                mask[1:].data_ptr() if outs != "counts" else None, counts.data_ptr() if outs != "mask" else None,
                                rets.data_ptr() if want_rets else None, stream()))
    torch.cuda.synchronize()
    m, k, r = mask.cpu().numpy(), counts.cpu().numpy(), rets.cpu().numpy()
    assert m[0] == sentinel and np.all(m[1 + n * MB:] == sentinel) and np.all(k[n:] == -77) and np.all(r[n:] == -7777), "written outside the outputs"
    if outs == "counts":
        assert np.all(m == sentinel), "a NULL mask was written"
    if outs == "mask":
        assert np.all(k == -77), "NULL counts were written"
    if not want_rets:
        assert np.all(r == -7777), "NULL rets were written"
    c, p, s = cls.cpu().numpy(), pos.cpu().numpy(), surv.cpu().numpy()
    assert np.all(c[n:] == 0x77) and np.all(p[n + 1:] == -0x1234) and np.all(s[n + 1:] == -0x4321), "prune wrote outside its outputs"
    return {"mask": m[1:1 + n * MB].reshape(n, MB), "counts": k[:n].astype(np.int64), "rets": r[:n], "class": c[:n], "pos": p[:n + 1], "surv": s[:n + 1],
            "survivors": ns}


def raw_plain_rets(cd, batch, codec, pred):
    """the unpruned entry point's rets"""
    import torch
    from sprintz_amd import _lib
    n, D, esz, chunk_len = batch.nchunks, cd.ndims, cd.esz, cd.chunk_len
    R, MB = fm.geometry(chunk_len, D)
    cid = _lib.CODEC_DELTA if codec == "delta" else _lib.CODEC_XFF
    mask = torch.empty(n * MB, dtype=torch.uint8, device="cuda")
    counts = torch.empty(n, dtype=torch.int32, device="cuda")
    rets = torch.empty(n, dtype=torch.int64, device="cuda")
    if pred[0] == "box":
        _lib.check(_lib.filter_rows(cid, esz, batch.data.data_ptr(), batch.offsets.data_ptr(), n, chunk_len, D, pred[1].data_ptr(), pred[2].data_ptr(), pred[3],
                                    0, mask.data_ptr(), counts.data_ptr(), rets.data_ptr(), stream()))
    else:
        _lib.check(_lib.filter_linear(cid, esz, batch.data.data_ptr(), batch.offsets.data_ptr(), n, chunk_len, D, pred[1].data_ptr(), None, pred[2], pred[3],
                                      pred[4], 0, None, mask.data_ptr(), counts.data_ptr(), rets.data_ptr(), stream()))
    torch.cuda.synchronize()
    return mask.cpu().numpy().reshape(n, MB), counts.cpu().numpy().astype(np.int64), rets.cpu().numpy()


def assert_prune_outputs(got, cls, offsets, msg):
    assert np.array_equal(got["class"], cls), ("class",) + msg
    assert np.array_equal(got["pos"], zm.positions(cls)), ("pos",) + msg
    assert np.array_equal(got["surv"], zm.surviving_offsets(cls, offsets)), ("surv",) + msg
    assert got["survivors"] == int((cls == zm.DECODE).sum()), msg


def check_python_call(cd, call, want, cls, msg):
    """call(zones) -> filter dict.  Without and with zones: the model's mask and counts; last_prune the model's classes; a decoder launch iff a chunk survives"""
    plain = call(None)
    ns = int((cls == zm.DECODE).sum())
    cd.last_prune = None
    with ran(**({"one_of": DECODERS} if ns else {"never": DECODERS})):
        got = call(True)
    for name, g in (("plain", plain), ("zones", got)):
        assert np.array_equal(g["mask"].cpu().numpy(), want[0]), (name, "mask") + msg
        assert np.array_equal(g["counts"].cpu().numpy().astype(np.int64), want[1]), (name, "counts") + msg
    lp = cd.last_prune
    assert lp["nchunks"] == len(cls) and lp["survivors"] == ns and np.array_equal(lp["class"].cpu().numpy(), cls), ("last_prune",) + msg


PARITY = [
    # (esz, D, chunk_len, family): test_gpu_linear.py's shapes
    (1, 8, 5120, 0), (2, 8, 5120, 0),
    (1, 80, 10240, 0),                # two columns a lane
    (2, 5, 5 * 104, 0),               # lanes with columns past the last
    (2, 3, 300, 0),                   # R = 100: MB = 13, the last mask byte partly padding, chunks at odd mask addresses
    (1, 4, 80, 0),                    # R = 20: MB = 3, the chunk is all verbatim tail
    (1, 1, 1024, 0),                  # decode_uni
    (2, 300, 9600, 0),                # the generic kernel
    (2, 8, 5120, 1),                  # the headline shape under OPT_NO_FAST
]
NCHUNKS = 37


@pytest.mark.parametrize("codec", ["delta", "xff"])
@pytest.mark.parametrize("esz,D,chunk_len,fam", PARITY)
def test_zone_parity(sz, oracle, no_fast, codec, esz, D, chunk_len, fam):
    rng = np.random.default_rng(zlib.crc32(f"zone{codec}{esz}{D}{chunk_len}{fam}".encode()))
    short = chunk_len // 3 + 1                                        # a short last chunk that ends mid-row (D = 1: mid-chunk)
    msg = (codec, esz, D, chunk_len, fam)
    no_fast(fam)
    # ---- box, on the levelled data as it is
    x = level_data(rng, NCHUNKS, chunk_len, esz, D, short)
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    offsets = batch.offsets.cpu().numpy()
    z = cd.zone_map(batch)
    zmin, zmax, zlen = assert_zone_map(z, x, chunk_len, D, esz, msg)
    for mode, name in ((fm.ALL, "all"), (fm.ANY, "any")):
        lo, hi = box_bounds(esz, D, mode)
        cls = zm.classify_box(zmin, zmax, zlen, lo, hi, mode, D)
        assert set(cls) == {zm.NONE, zm.ALL, zm.DECODE}, ("the inputs must produce every class", name) + msg
        want = fm.filter_rows(x, chunk_len, D, lo, hi, mode)
        check_python_call(cd, lambda zones: cd.filter_rows(batch, list(map(int, lo)), list(map(int, hi)), mode=name, zones=z if zones else None),
                          want, cls, (name,) + msg)
        pred = ("box", dev(lo.astype(DTYPES[esz])), dev(hi.astype(DTYPES[esz])), mode)
        got = raw_zoned(sz, cd, batch, codec, z, pred)
        pm, pk, pr = raw_plain_rets(cd, batch, codec, pred)
        assert_prune_outputs(got, cls, offsets, (name,) + msg)
        assert np.array_equal(got["mask"], want[0]) and np.array_equal(got["counts"], want[1]), ("raw", name) + msg
        assert np.array_equal(got["mask"], pm) and np.array_equal(got["counts"], pk) and np.array_equal(got["rets"], pr), ("raw against unpruned", name) + msg
        assert np.array_equal(got["rets"], zlen), ("rets", name) + msg
    # ---- linear: "ones" on the same data; "a - b" on data whose last column stays at level 0, so that the difference follows the levels
    ones = np.ones(D, np.int64)
    e = np.eye(D, dtype=np.int64)
    x2 = level_data(rng, NCHUNKS, chunk_len, esz, D, short, flat_last_column=True)
    cd2, batch2 = make_batch(sz, oracle, codec, esz, D, chunk_len, x2, False)
    z2 = cd2.zone_map(batch2)
    zone2 = assert_zone_map(z2, x2, chunk_len, D, esz, msg)
    for name, c_, b_, z_, xx, zone, w, lo, hi in (("ones", cd, batch, z, x, (zmin, zmax, zlen), ones, BAND[0] * D, BAND[1] * D),
                                                  ("a - b", cd2, batch2, z2, x2, zone2, e[0] - e[D - 1] if D > 1 else e[0], 80, 120)):
        cls = zm.classify_linear(*zone, w, 0, lo, hi, D)
        assert set(cls) == {zm.NONE, zm.ALL, zm.DECODE}, ("the inputs must produce every class", name) + msg
        want = lm.filter_linear(xx, chunk_len, D, w, lo, hi)
        check_python_call(c_, lambda zones: c_.filter_linear(b_, [int(v) for v in w], lo=lo, hi=hi, zones=z_ if zones else None), want, cls, (name,) + msg)
        pred = ("lin", dev(w.astype(np.int32)), 0, lo, hi)
        got = raw_zoned(sz, c_, b_, codec, z_, pred)
        pm, pk, pr = raw_plain_rets(c_, b_, codec, pred)
        assert_prune_outputs(got, cls, b_.offsets.cpu().numpy(), (name,) + msg)
        assert np.array_equal(got["mask"], want[0]) and np.array_equal(got["counts"], want[1]), ("raw", name) + msg
        assert np.array_equal(got["mask"], pm) and np.array_equal(got["counts"], pk) and np.array_equal(got["rets"], pr), ("raw against unpruned", name) + msg


@pytest.mark.parametrize("codec,esz,D,chunk_len", [("xff", 2, 8, 5120), ("delta", 2, 3, 300), ("delta", 1, 4, 80)])
def test_zone_edges(sz, oracle, codec, esz, D, chunk_len):
    """every chunk pruned (no decoder launch at all), none pruned, batches of one and two chunks, a short last chunk of every class, and the
    mask-only and counts-only outputs"""
    rng = np.random.default_rng(esz * 100 + D)
    top = (1 << (8 * esz)) - 1
    short = chunk_len // 3 + 1
    R, MB = fm.geometry(chunk_len, D)
    for nchunks in (1, 2, 37, 38, 39, 40):                            # the short last chunk is at level 0, 100, 0, 100, 110, 200: NONE, ALL, DECODE
        x = level_data(rng, nchunks, chunk_len, esz, D, short)
        cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
        z = cd.zone_map(batch)
        zmin, zmax, zlen = assert_zone_map(z, x, chunk_len, D, esz, (nchunks,))
        sets = [("band", fm.ALL) + box_bounds(esz, D, fm.ALL), ("band any", fm.ANY) + box_bounds(esz, D, fm.ANY),
                ("nothing", fm.ALL, np.full(D, 250, np.int64), np.full(D, top, np.int64)),                 # every chunk NONE
                ("everything", fm.ALL, np.zeros(D, np.int64), np.full(D, top, np.int64)),                  # every chunk ALL
                ("never", fm.ANY, np.full(D, top, np.int64), np.zeros(D, np.int64)),                       # lo > hi in every column
                ("across", fm.ALL, np.full(D, 5, np.int64), np.full(D, 205, np.int64))]                    # levels 0 and 200 straddle, the others lie inside
        for name, mode, lo, hi in sets:
            cls = zm.classify_box(zmin, zmax, zlen, lo, hi, mode, D)
            if name in ("nothing", "never"):
                assert set(cls) == {zm.NONE}
            if name == "everything":
                assert set(cls) == {zm.ALL}
            want = fm.filter_rows(x, chunk_len, D, lo, hi, mode)
            check_python_call(cd, lambda zones: cd.filter_rows(batch, list(map(int, lo)), list(map(int, hi)), mode="all" if mode == fm.ALL else "any",
                                                               zones=z if zones else None), want, cls, (nchunks, name))
            if nchunks in (2, 39):
                pred = ("box", dev(lo.astype(DTYPES[esz])), dev(hi.astype(DTYPES[esz])), mode)
                for outs, rets in (("mask", True), ("counts", True), ("both", False)):
                    got = raw_zoned(sz, cd, batch, codec, z, pred, outs=outs, want_rets=rets, sentinel=0xA5 if outs == "mask" else 0x5A)
                    if outs != "counts":
                        assert np.array_equal(got["mask"], want[0]), (nchunks, name, outs)
                    if outs != "mask":
                        assert np.array_equal(got["counts"], want[1]), (nchunks, name, outs)
                    if rets:
                        assert np.array_equal(got["rets"], zlen), (nchunks, name, outs)
    # none pruned: every chunk of uniform data reaches across both ends of the type's middle half
    nchunks = 9
    x = gen_data("uniform", rng, nchunks * chunk_len - short, esz, D)
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    z = cd.zone_map(batch)
    zmin, zmax, zlen = assert_zone_map(z, x, chunk_len, D, esz, ("uniform",))
    lo, hi = np.full(D, top // 4, np.int64), np.full(D, 3 * (top // 4), np.int64)
    cls = zm.classify_box(zmin, zmax, zlen, lo, hi, fm.ALL, D)
    assert set(cls) == {zm.DECODE}
    check_python_call(cd, lambda zones: cd.filter_rows(batch, list(map(int, lo)), list(map(int, hi)), zones=z if zones else None),
                      fm.filter_rows(x, chunk_len, D, lo, hi, fm.ALL), cls, ("uniform",))


@pytest.mark.parametrize("nchunks", [17, 1025, 16385])
def test_zone_scan_tiles(sz, oracle, nchunks):
    """one chunk past each tile edge of the size scan that places the survivors: 16 sizes a thread, 1 024 a wavefront of the one-workgroup scan,
    16 384 chunks from which the three-launch scan of 1 024-chunk blocks takes over -- with 64-element 8-bit chunks"""
    esz, D, chunk_len, codec = 1, 4, 64, "delta"
    rng = np.random.default_rng(nchunks)
    x = level_data(rng, nchunks, chunk_len, esz, D, 9)
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    z = cd.zone_map(batch)
    zmin, zmax, zlen = assert_zone_map(z, x, chunk_len, D, esz, (nchunks,))
    lo, hi = box_bounds(esz, D, fm.ALL)
    cls = zm.classify_box(zmin, zmax, zlen, lo, hi, fm.ALL, D)
    assert set(cls) == {zm.NONE, zm.ALL, zm.DECODE}
    want = fm.filter_rows(x, chunk_len, D, lo, hi, fm.ALL)
    check_python_call(cd, lambda zones: cd.filter_rows(batch, list(map(int, lo)), list(map(int, hi)), zones=z if zones else None), want, cls, (nchunks,))
    got = raw_zoned(sz, cd, batch, codec, z, ("box", dev(lo.astype(np.uint8)), dev(hi.astype(np.uint8)), fm.ALL))
    assert_prune_outputs(got, cls, batch.offsets.cpu().numpy(), (nchunks,))
    assert np.array_equal(got["mask"], want[0]) and np.array_equal(got["counts"], want[1]) and np.array_equal(got["rets"], zlen)


@pytest.mark.parametrize("codec,esz,D,chunk_len,fam", [("xff", 2, 8, 5120, 0), ("delta", 1, 1, 1024, 0), ("xff", 2, 8, 5120, 1)])
def test_zone_damaged_chunk(sz, oracle, no_fast, codec, esz, D, chunk_len, fam):
    """a stream damaged before zone_map: its zlen is negative, so it is DECODE whatever its bounds say, and the decoder reports it under its
    batch number with the code the unpruned call gives"""
    no_fast(fam)
    rng = np.random.default_rng(7)
    nchunks, bad = 13, 4                                              # chunk 4 is at level 0: NONE, were it whole
    x = level_data(rng, nchunks, chunk_len, esz, D, 100)
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    off = int(batch.offsets[bad].item())
    hdr = batch.data[off + 6:off + 8].clone()
    batch.data[off + 6] = hdr[0] ^ 0x5                                # the header's ndims field
    z = cd.zone_map(batch)
    zlen_got = host(z.len)
    zmin, zmax, zlen = zm.zone_map(x, chunk_len, D, esz)
    assert zlen_got[bad] < 0 and np.array_equal(np.delete(zlen_got, bad), np.delete(zlen, bad))
    zlen_d = zlen.copy()
    zlen_d[bad] = zlen_got[bad]
    lo, hi = box_bounds(esz, D, fm.ALL)
    cls = zm.classify_box(zmin, zmax, zlen_d, lo, hi, fm.ALL, D)
    assert cls[bad] == zm.DECODE and zm.classify_box(zmin, zmax, zlen, lo, hi, fm.ALL, D)[bad] == zm.NONE
    want = fm.filter_rows(x, chunk_len, D, lo, hi, fm.ALL)
    pred = ("box", dev(lo.astype(DTYPES[esz])), dev(hi.astype(DTYPES[esz])), fm.ALL)
    got = raw_zoned(sz, cd, batch, codec, z, pred)
    pm, pk, pr = raw_plain_rets(cd, batch, codec, pred)
    assert np.array_equal(got["class"], cls)
    assert pr[bad] < 0 and np.array_equal(got["rets"], pr)           # the same negative ret as unpruned, every other chunk's element count
    keep = np.arange(nchunks) != bad
    assert np.array_equal(got["mask"][keep], want[0][keep]) and np.array_equal(got["counts"][keep], want[1][keep])
    with pytest.raises(sz.SprintzError, match=f"chunk {bad} "):
        cd.filter_rows(batch, list(map(int, lo)), list(map(int, hi)), zones=z, check=True)
    res = cd.filter_rows(batch, list(map(int, lo)), list(map(int, hi)), zones=z, check=False)
    assert np.array_equal(res["mask"].cpu().numpy()[keep], want[0][keep])
    with pytest.raises(sz.SprintzError, match=f"chunk {bad} "):
        cd.filter_rows(batch, list(map(int, lo)), list(map(int, hi)), zones=z, ids=True, check=False)
    batch.data[off + 6] = hdr[0]


@pytest.mark.parametrize("codec,esz,D,chunk_len,fam", [("xff", 2, 8, 5120, 0), ("delta", 1, 80, 10240, 0), ("delta", 1, 1, 1024, 0), ("xff", 2, 8, 5120, 1)])
def test_zone_truncated_chunk(sz, oracle, no_fast, codec, esz, D, chunk_len, fam):
    """A stream cut short by 5 bytes and the streams packed densely again (as test_gpu_extrema.py truncates them), with the chunk behind it
    pruned.  A decoder tells a truncated stream by its length alone, and in the survivors' container that length runs on over the pruned
    neighbour's bytes: the zoned call must still report the chunk, with the code the unpruned call gives, from the map"""
    import torch
    no_fast(fam)
    rng = np.random.default_rng(13)
    nchunks = 13
    x = level_data(rng, nchunks, chunk_len, esz, D, 100 if D > 1 else 7)
    cd, whole = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    lo, hi = box_bounds(esz, D, fm.ALL)
    zmin, zmax, zlen = zm.zone_map(x, chunk_len, D, esz)
    comp0, offs, sizes = whole.data.cpu().numpy().copy(), whole.offsets.cpu().numpy(), whole.sizes.cpu().numpy()
    for bad in (2, 4, 9):                                             # at levels 110, 0, 100: DECODE, NONE, ALL were they whole; the chunk behind is NONE, ALL, DECODE
        parts = [comp0[offs[c]:offs[c] + sizes[c] - (5 if c == bad else 0)] for c in range(nchunks)]
        toffs = np.zeros(nchunks + 1, np.int64)
        toffs[1:] = np.cumsum([p.size for p in parts])
        data = torch.from_numpy(np.concatenate(parts + [np.zeros(sz._lib.READ_SLACK, np.uint8)])).cuda()
        batch = sz.CompressedBatch(data, torch.from_numpy(toffs).cuda(), torch.tensor([p.size for p in parts], dtype=torch.int32).cuda(), nchunks, x.size,
                                   chunk_len, D)
        z = cd.zone_map(batch)
        zlen_got = host(z.len)
        assert zlen_got[bad] < 0 and np.array_equal(np.delete(zlen_got, bad), np.delete(zlen, bad)), bad
        zlen_d = zlen.copy()
        zlen_d[bad] = zlen_got[bad]
        cls = zm.classify_box(zmin, zmax, zlen_d, lo, hi, fm.ALL, D)
        assert cls[bad] == zm.DECODE and {zm.NONE, zm.ALL, zm.DECODE} == set(cls)
        if bad != 9:
            assert cls[bad + 1] != zm.DECODE                          # the stretched length covers a pruned chunk's bytes
        want = fm.filter_rows(x, chunk_len, D, lo, hi, fm.ALL)
        pred = ("box", dev(lo.astype(DTYPES[esz])), dev(hi.astype(DTYPES[esz])), fm.ALL)
        got = raw_zoned(sz, cd, batch, codec, z, pred)
        pm, pk, pr = raw_plain_rets(cd, batch, codec, pred)
        assert pr[bad] < 0 and np.array_equal(got["rets"], pr), (bad, got["rets"], pr)
        assert np.array_equal(got["class"], cls), bad
        keep = np.arange(nchunks) != bad
        assert np.array_equal(got["mask"][keep], want[0][keep]) and np.array_equal(got["counts"][keep], want[1][keep]), bad
        assert np.array_equal(pm[keep], want[0][keep]) and np.array_equal(pk[keep], want[1][keep]), bad
        with pytest.raises(sz.SprintzError, match=f"chunk {bad} "):
            cd.filter_rows(batch, list(map(int, lo)), list(map(int, hi)), zones=z, check=True)
        res = cd.filter_rows(batch, list(map(int, lo)), list(map(int, hi)), zones=z, check=False)
        assert np.array_equal(res["mask"].cpu().numpy()[keep], want[0][keep]), bad


def assert_same(a, b, msg):
    """two results of one operation -- tensors, or dicts / tuples of them -- are equal (NaN equals NaN)"""
    import torch
    if isinstance(a, dict):
        assert set(a) == set(b), msg
        for k in a:
            assert_same(a[k], b[k], msg + (k,))
    elif isinstance(a, (tuple, list)):
        assert len(a) == len(b), msg
        for i, (u, v) in enumerate(zip(a, b)):
            assert_same(u, v, msg + (i,))
    elif torch.is_tensor(a):
        if a.dtype.is_floating_point:
            assert np.array_equal(a.cpu().numpy(), b.cpu().numpy(), equal_nan=True), msg
        else:
            assert np.array_equal(host(a), host(b)), msg
    else:
        assert a == b, msg


def test_zone_python_surface(sz, oracle):
    """filter_linear with a lag term ignores the zones; a map built under the other layout flag or quirk state is refused; the *_where operations
    pass their zones to the filter step and return what they return without"""
    from sprintz_amd import _lib
    codec, esz, D, chunk_len = "xff", 2, 8, 5120
    rng = np.random.default_rng(11)
    x = level_data(rng, 12, chunk_len, esz, D, 8 * 100)
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    z = cd.zone_map(batch)
    # lag + zones: the unpruned call, whatever the map says
    w = {0: 1}
    cd.last_prune = None
    a = cd.filter_linear(batch, w, lo=-3, hi=3, lag_weights={0: -1})
    b = cd.filter_linear(batch, w, lo=-3, hi=3, lag_weights={0: -1}, zones=z)
    want = lm.filter_linear(x, chunk_len, D, np.eye(D, dtype=np.int64)[0], -3, 3, -np.eye(D, dtype=np.int64)[0])
    for g in (a, b):
        assert np.array_equal(g["mask"].cpu().numpy(), want[0]) and np.array_equal(g["counts"].cpu().numpy().astype(np.int64), want[1])
    assert cd.last_prune is None
    cd.filter_rows(batch, [BAND[0]] * D, [BAND[1]] * D, zones=z)
    assert cd.last_prune["survivors"] == 3
    cd.filter_linear(batch, w, lo=-3, hi=3, lag_weights={0: -1}, zones=z)       # what an earlier call pruned is not this call's
    assert cd.last_prune is None
    cd.filter_rows(batch, [BAND[0]] * D, [BAND[1]] * D, zones=z)
    cd.filter_rows(batch, [BAND[0]] * D, [BAND[1]] * D)
    assert cd.last_prune is None
    # a map of another layout flag, of another quirk state, of another batch
    lo, hi = [BAND[0]] * D, [BAND[1]] * D
    zg = cd.zone_map(batch, general_layout=True)
    with pytest.raises(ValueError, match="general_layout"):
        cd.filter_rows(batch, lo, hi, zones=zg)
    with pytest.raises(ValueError, match="general_layout"):
        cd.filter_linear(batch, 1, lo=0, zones=zg)
    with pytest.raises(ValueError, match="general_layout"):          # a lag term ignores a map only after it was found to be this call's
        cd.filter_linear(batch, w, lo=-3, hi=3, lag_weights={0: -1}, zones=zg)
    cd.filter_rows(batch, lo, hi, general_layout=True, zones=zg)
    try:
        _lib.check(_lib.set_option(_lib.OPT_REF_DECODER_QUIRK, 1))
        with pytest.raises(ValueError, match="QUIRK"):
            cd.filter_rows(batch, lo, hi, zones=z)
        zq = cd.zone_map(batch)
        assert zq.quirk == 1
        cd.filter_rows(batch, lo, hi, zones=zq)
    finally:
        _lib.set_option(_lib.OPT_REF_DECODER_QUIRK, 0)
    x3 = level_data(rng, 5, chunk_len, esz, D, 0)
    cd3, batch3 = make_batch(sz, oracle, codec, esz, D, chunk_len, x3, False)
    with pytest.raises(ValueError, match="chunks"):
        cd.filter_rows(batch, lo, hi, zones=cd3.zone_map(batch3))
    # the *_where operations
    cd.last_prune = None
    r0, r1 = cd.where(batch, lo, hi, ids=True), cd.where(batch, lo, hi, ids=True, zones=z)
    assert cd.last_prune is not None and 0 < cd.last_prune["survivors"] < batch.nchunks
    assert np.array_equal(host(r0["rows"]), host(r1["rows"])) and np.array_equal(r0["ids"].cpu().numpy(), r1["ids"].cpu().numpy()) and r0["ids"].numel() > 0
    for name, kw in (("aggregate_where", {}), ("histogram_where", {"nbins": 16}), ("moments_where", {}), ("extrema_where", {}), ("groupby_where", {"key": 0, "nbins": 16})):
        f = getattr(cd, name)
        assert_same(f(batch, lo, hi, **kw), f(batch, lo, hi, zones=z, **kw), (name,))


def test_zone_c_abi(sz):
    """prune needs no container: hand-made offsets and zones.  The span rule on both sides of 0xf0000000, garbage in the outputs beforehand, one
    chunk past the tile of the scan's middle launch (1 024 blocks of 1 024 chunks), and refusals that leave the outputs alone"""
    import torch
    from sprintz_amd import _lib, rowops
    esz, D, chunk_len = 1, 2, 64
    n = 9
    zmin = np.array([[0, 0], [100, 100], [110, 110], [200, 200], [0, 0], [100, 100], [110, 110], [200, 200], [95, 95]], np.uint8)
    zmax = zmin + 15
    zlen = np.full(n, chunk_len, np.int64)
    zlen[4], zlen[5] = -5, 1                                          # a damaged chunk (at a NONE level) and one without a whole row (at the ALL level)
    lo, hi = np.full(D, BAND[0], np.uint8), np.full(D, BAND[1], np.uint8)
    for span in (zm.SPAN_LIMIT - 1, zm.SPAN_LIMIT, zm.SPAN_LIMIT + 4096):
        offsets = np.concatenate([np.arange(n) * 16 + 4096, [4096 + span]]).astype(np.int64)
        cls = zm.classify_box(zmin, zmax, zlen, lo, hi, fm.ALL, D, span)
        if span >= zm.SPAN_LIMIT:
            assert set(cls) == {zm.DECODE}
        else:
            assert list(cls) == [zm.NONE, zm.ALL, zm.DECODE, zm.NONE, zm.DECODE, zm.NONE, zm.DECODE, zm.NONE, zm.ALL]
        t_cls = torch.full((n + 8,), 0x77, dtype=torch.uint8, device="cuda")
        t_pos = torch.full((n + 1 + 4,), -0x1234, dtype=torch.int64, device="cuda")
        t_surv = torch.full((n + 1 + 4,), -0x4321, dtype=torch.int64, device="cuda")
        tmp = torch.full((_lib.zone_prune_tmp_bytes(n) // 8,), -1, dtype=torch.int64, device="cuda")
        keep = [dev(offsets), dev(zmin), dev(zmax), dev(zlen), dev(lo), dev(hi)]
        args = (esz, n, chunk_len, D) + tuple(t.data_ptr() for t in keep[:4])
        _lib.check(_lib.zone_prune_box(*args, keep[4].data_ptr(), keep[5].data_ptr(), fm.ALL, t_cls.data_ptr(), t_pos.data_ptr(), t_surv.data_ptr(),
                                       tmp.data_ptr(), stream()))
        torch.cuda.synchronize()
        c, p, s = t_cls.cpu().numpy(), t_pos.cpu().numpy(), t_surv.cpu().numpy()
        assert np.array_equal(c[:n], cls) and np.all(c[n:] == 0x77), span
        assert np.array_equal(p[:n + 1], zm.positions(cls)) and np.all(p[n + 1:] == -0x1234), span
        assert np.array_equal(s[:n + 1], zm.surviving_offsets(cls, offsets)) and np.all(s[n + 1:] == -0x4321), span
        # the linear form x0 + x1 in 2 * BAND: the same classes
        w = dev(np.ones(D, np.int32))
        t_cls.fill_(0x77)
        _lib.check(_lib.zone_prune_linear(*args, w.data_ptr(), 0, 2 * BAND[0], 2 * BAND[1], t_cls.data_ptr(), t_pos.data_ptr(), t_surv.data_ptr(),
                                          tmp.data_ptr(), stream()))
        torch.cuda.synchronize()
        assert np.array_equal(t_cls.cpu().numpy()[:n], zm.classify_linear(zmin, zmax, zlen, np.ones(D, np.int64), 0, 2 * BAND[0], 2 * BAND[1], D, span)), span
        assert np.array_equal(t_pos.cpu().numpy()[:n + 1], zm.positions(cls)), span
        # refusals leave the outputs alone
        t_cls.fill_(0x77)
        assert _lib.zone_prune_box(*args, keep[4].data_ptr(), keep[5].data_ptr(), 2, t_cls.data_ptr(), t_pos.data_ptr(), t_surv.data_ptr(), tmp.data_ptr(),
                                   stream()) == _lib.E_INVALID
        assert _lib.zone_prune_box(*args, keep[4].data_ptr(), keep[5].data_ptr(), fm.ALL, t_cls.data_ptr(), t_pos.data_ptr() + 4, t_surv.data_ptr(),
                                   tmp.data_ptr(), stream()) == _lib.E_INVALID
        assert _lib.zone_prune_linear(esz, n, chunk_len + 1, D, *args[4:], w.data_ptr(), 0, 0, 1, t_cls.data_ptr(), t_pos.data_ptr(), t_surv.data_ptr(),
                                      tmp.data_ptr(), stream()) == _lib.E_INVALID
        assert _lib.zone_expand(n, chunk_len, D, t_cls.data_ptr(), t_pos.data_ptr(), keep[3].data_ptr(), None, None, None, None, None, None, stream()) == _lib.E_INVALID
        torch.cuda.synchronize()
        assert np.all(t_cls.cpu().numpy() == 0x77)
    # 1 024 * 1 024 + 1 chunks of one 8-bit column: the scan's middle launch walks a second tile of block sums
    n, D = 1024 * 1024 + 1, 1
    rng = np.random.default_rng(3)
    level = np.array(LEVELS, np.int64)[rng.integers(0, 4, n)]
    zmin = level.astype(np.uint8).reshape(n, 1)
    zmax = zmin + 15
    zlen = np.full(n, chunk_len, np.int64)
    offsets = (np.arange(n + 1, dtype=np.int64) * 80)
    lo, hi = np.full(D, BAND[0], np.uint8), np.full(D, BAND[1], np.uint8)
    t = lambda a: torch.from_numpy(a.astype(np.int64))               # noqa: E731
    cls = rowops.zone_classify_box(t(zmin), t(zmax), t(zlen), t(lo), t(hi), "all", chunk_len, D, int(offsets[-1] - offsets[0])).numpy()
    assert set(cls) == {zm.NONE, zm.ALL, zm.DECODE}
    keep = [dev(offsets), dev(zmin), dev(zmax), dev(zlen), dev(lo), dev(hi)]
    t_cls = torch.full((n,), 0x77, dtype=torch.uint8, device="cuda")
    t_pos = torch.full((n + 1,), -0x1234, dtype=torch.int64, device="cuda")
    t_surv = torch.full((n + 1,), -0x4321, dtype=torch.int64, device="cuda")
    tmp = torch.full((_lib.zone_prune_tmp_bytes(n) // 8,), -1, dtype=torch.int64, device="cuda")
    _lib.check(_lib.zone_prune_box(esz, n, chunk_len, D, *(k.data_ptr() for k in keep[:4]), keep[4].data_ptr(), keep[5].data_ptr(), fm.ALL, t_cls.data_ptr(),
                                   t_pos.data_ptr(), t_surv.data_ptr(), tmp.data_ptr(), stream()))
    torch.cuda.synchronize()
    assert np.array_equal(t_cls.cpu().numpy(), cls)
    assert np.array_equal(t_pos.cpu().numpy(), zm.positions(cls))
    assert np.array_equal(t_surv.cpu().numpy(), zm.surviving_offsets(cls, offsets))
