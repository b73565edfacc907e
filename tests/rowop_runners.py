"""One runner per row operation, for its own GPU tests and for the drives that run every operation over one batch: run_* calls the C entry
point on sentinel-filled outputs, check_* compares what it wrote with the operation's numpy model and asserts that nothing else was written."""
import ctypes as C

import numpy as np

import aggregate_model as am
import extrema_model as em
import filter_model as fm
import groupby_model as gm
import histogram_model as hm
import moments_model as mm
import select_model as sm
import zone_model as zm
from fixtures import sentinel, sentinels
from harness import DTYPES


# ------------------------------------------------------------------ the filter's

def run_filter(cd, batch, lo, hi, mode, general=False):
    got = cd.filter_rows(batch, [int(v) for v in lo], [int(v) for v in hi], mode="all" if mode == fm.ALL else "any", general_layout=general)
    return got["mask"].cpu().numpy(), got["counts"].cpu().numpy().astype(np.int64)


# ------------------------------------------------------------------ select rows'

PAD = 4096                      # elements behind both outputs that must keep the sentinel


def run_select(batch, codec, esz, D, chunk_len, mask, bases, capacity, out_rows, byte=0x5A, ids=True, general=False, shift=0):
    """the C entry point on sentinel-filled outputs of out_rows rows + PAD elements (the rows start `shift` elements into their buffer)
    -> (rows [out_rows * D + PAD] numpy, ids [out_rows + PAD] numpy int64, rets [nchunks] numpy)"""
    import torch
    from sprintz_amd import _lib
    n = batch.nchunks
    elem, ident = sentinels(esz, byte)
    ne = out_rows * D + PAD
    rows_t = torch.from_numpy(np.full(ne + shift, elem, DTYPES[esz]).view(np.int8 if esz == 1 else np.int16)).cuda()
    ids_t = torch.full((out_rows + PAD,), ident, dtype=torch.int64, device="cuda")
    rets_t = torch.full((n + 1,), -77, dtype=torch.int64, device="cuda")
    mask_t = torch.from_numpy(np.ascontiguousarray(mask, np.uint8)).cuda()
    bases_t = torch.from_numpy(np.ascontiguousarray(bases, np.int64)).cuda()
    _lib.check(_lib.select_rows(_lib.CODEC_DELTA if codec == "delta" else _lib.CODEC_XFF, esz, batch.data.data_ptr(), batch.offsets.data_ptr(),
                                n, chunk_len, D, mask_t.data_ptr(), bases_t.data_ptr(), int(capacity), _lib.QUERY_GENERAL_LAYOUT if general else 0,
                                rows_t.data_ptr() + shift * esz, ids_t.data_ptr() if ids else None, rets_t.data_ptr(),
                                C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    r = rets_t.cpu().numpy()
    assert r[n] == -77, "rets written past nchunks"
    got = rows_t.cpu().numpy().view(DTYPES[esz])
    assert np.all(got[:shift] == elem), "written in front of d_out"
    return got[shift:], ids_t.cpu().numpy(), r[:n]


def check_select(x, batch, codec, esz, D, chunk_len, mask, bases, capacity, out_rows, msg, byte=0x5A, ids=True, general=False, shift=0):
    """rows, ids, padding and rets against the model"""
    elem, ident = sentinels(esz, byte)
    want_rows, want_ids = sm.select_rows(x, chunk_len, D, mask, bases, capacity, out_rows=out_rows, sentinel=elem, id_sentinel=ident)
    rows, got_ids, rets = run_select(batch, codec, esz, D, chunk_len, mask, bases, capacity, out_rows, byte, ids, general, shift)
    assert np.array_equal(rets, fm.chunk_counts(x.size, chunk_len)), ("rets",) + msg
    assert np.all(rows[out_rows * D:] == elem) and np.all(got_ids[out_rows:] == ident), ("padding",) + msg
    assert np.array_equal(rows[:out_rows * D].reshape(out_rows, D), want_rows), ("rows",) + msg
    if ids:
        assert np.array_equal(got_ids[:out_rows], want_ids), ("ids",) + msg
    else:
        assert np.all(got_ids == ident), ("a NULL d_ids was written",) + msg
    return want_rows, want_ids


# ------------------------------------------------------------------ aggregate rows' (and the other masked operations')

AGG_PAD = 1024                      # entries behind every output that must keep the sentinel
OPS = {"min": 1, "max": 2, "sum": 4, "count": 8}


def run_agg(batch, codec, esz, D, chunk_len, mask, W, ops=15, byte=0x5A, general=False, mask_shift=0, null_unselected=False):
    """the C entry point on sentinel-filled outputs of nchunks * nwin (* D) entries + PAD -> ({op: numpy incl. padding}, rets [nchunks])"""
    import torch
    from sprintz_amd import _lib
    n = batch.nchunks
    R = chunk_len // D
    nwin = -(-R // W)
    m = n * nwin
    elem = sentinel(esz, byte)
    bufs = {
        "min": torch.from_numpy(np.full(m * D + AGG_PAD, elem, DTYPES[esz]).view(np.int8 if esz == 1 else np.int16)).cuda(),
        "max": torch.from_numpy(np.full(m * D + AGG_PAD, elem, DTYPES[esz]).view(np.int8 if esz == 1 else np.int16)).cuda(),
        "sum": torch.from_numpy(np.full(m * D + AGG_PAD, sentinel(8, byte), np.uint64).view(np.int64)).cuda(),
        "count": torch.from_numpy(np.full(m + AGG_PAD, sentinel(4, byte), np.uint32).view(np.int32)).cuda(),
    }
    rets_t = torch.full((n + 1,), -77, dtype=torch.int64, device="cuda")
    flat = np.ascontiguousarray(mask, np.uint8).reshape(-1)
    mask_t = torch.from_numpy(np.concatenate([np.full(mask_shift, 0xFF, np.uint8), flat, np.full(16, 0xFF, np.uint8)])).cuda()

    def ptr(k):
        return None if null_unselected and not ops & OPS[k] else bufs[k].data_ptr()
    _lib.check(_lib.aggregate_rows(_lib.CODEC_DELTA if codec == "delta" else _lib.CODEC_XFF, esz, batch.data.data_ptr(), batch.offsets.data_ptr(),
                                   n, chunk_len, D, mask_t.data_ptr() + mask_shift, W, ops, _lib.QUERY_GENERAL_LAYOUT if general else 0,
                                   ptr("min"), ptr("max"), ptr("sum"), ptr("count"), rets_t.data_ptr(),
                                   C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    r = rets_t.cpu().numpy()
    assert r[n] == -77, "rets written past nchunks"
    got = {"min": bufs["min"].cpu().numpy().view(DTYPES[esz]), "max": bufs["max"].cpu().numpy().view(DTYPES[esz]),
           "sum": bufs["sum"].cpu().numpy().view(np.uint64), "count": bufs["count"].cpu().numpy().view(np.uint32)}
    return got, r[:n]


def check_agg(x, batch, codec, esz, D, chunk_len, mask, W, msg, want=None, ops=15, byte=0x5A, skip_chunk=None, **kw):
    """every selected output, the unselected ones, the padding and rets against the model; skip_chunk: a damaged chunk, whose own entries
    are unspecified"""
    want = am.aggregate_rows(x, chunk_len, D, mask, W) if want is None else want
    got, rets = run_agg(batch, codec, esz, D, chunk_len, mask, W, ops, byte, **kw)
    lens = np.array(fm.chunk_counts(x.size, chunk_len))
    keep = np.arange(batch.nchunks) != (-1 if skip_chunk is None else skip_chunk)
    assert np.array_equal(rets[keep], lens[keep]), ("rets",) + msg
    if skip_chunk is not None:
        assert rets[skip_chunk] < 0, ("rets of the damaged chunk",) + msg
    for k in ("min", "max", "sum", "count"):
        w = want[k]
        sent = sentinel({"sum": 8, "count": 4}.get(k, esz), byte)
        g = got[k]
        assert np.all(g[w.size:] == sent), (k, "padding") + msg
        g = g[:w.size].reshape(w.shape)
        if ops & OPS[k]:
            assert np.array_equal(g[keep], w[keep]), (k,) + msg
        else:
            assert np.all(g == sent), (k, "an unselected output was written") + msg
    return want


# ------------------------------------------------------------------ histogram and group-by rows'

HIST_PAD = 1024                      # entries behind d_hist that must keep the sentinel
SENT = 0x5A5A5A5A5A5A5A5A


def run_hist(batch, codec, esz, D, chunk_len, mask, lo, shift, nbins, H, general=False, mask_shift=0):
    """the C entry point on a sentinel-filled d_hist of ngroups * D * nbins entries + PAD -> (numpy uint64 incl. padding, rets [nchunks])"""
    import torch
    from sprintz_amd import _lib
    n = batch.nchunks
    ngroups = -(-n // H) if H else 1
    hist_t = torch.from_numpy(np.full(ngroups * D * nbins + HIST_PAD, SENT, np.uint64).view(np.int64)).cuda()
    rets_t = torch.full((n + 1,), -77, dtype=torch.int64, device="cuda")
    mask_ptr = None
    if mask is not None:
        flat = np.ascontiguousarray(mask, np.uint8).reshape(-1)
        mask_t = torch.from_numpy(np.concatenate([np.full(mask_shift, 0xFF, np.uint8), flat, np.full(16, 0xFF, np.uint8)])).cuda()
        mask_ptr = mask_t.data_ptr() + mask_shift
    lo_ptr = None
    if lo is not None:
        lo_t = torch.from_numpy(np.asarray(lo).astype(DTYPES[esz]).view(np.int8 if esz == 1 else np.int16)).cuda()
        lo_ptr = lo_t.data_ptr()
    _lib.check(_lib.histogram_rows(_lib.CODEC_DELTA if codec == "delta" else _lib.CODEC_XFF, esz, batch.data.data_ptr(), batch.offsets.data_ptr(),
                                   n, chunk_len, D, mask_ptr, lo_ptr, shift, nbins, H, _lib.QUERY_GENERAL_LAYOUT if general else 0,
                                   hist_t.data_ptr(), rets_t.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    r = rets_t.cpu().numpy()
    assert r[n] == -77, "rets written past nchunks"
    return hist_t.cpu().numpy().view(np.uint64), r[:n]


def check_hist(x, batch, codec, esz, D, chunk_len, mask, lo, shift, nbins, H, msg, want=None, skip_group=None, bad_chunk=None, **kw):
    """d_hist, its padding and rets against the model; skip_group: a damaged chunk's histogram, which is unspecified"""
    want = hm.histogram_rows(x, chunk_len, D, mask, lo, shift, nbins, H) if want is None else want
    got, rets = run_hist(batch, codec, esz, D, chunk_len, mask, lo, shift, nbins, H, **kw)
    lens = np.array(fm.chunk_counts(x.size, chunk_len))
    keep_c = np.arange(batch.nchunks) != (-1 if bad_chunk is None else bad_chunk)
    assert np.array_equal(rets[keep_c], lens[keep_c]), ("rets",) + msg
    if bad_chunk is not None:
        assert rets[bad_chunk] < 0, ("rets of the damaged chunk",) + msg
    assert np.all(got[want.size:] == SENT), ("padding",) + msg
    g = got[:want.size].reshape(want.shape)
    keep_g = np.arange(want.shape[0]) != (-1 if skip_group is None else skip_group)
    assert np.array_equal(g[keep_g], want[keep_g]), ("hist",) + msg
    return want


# ------------------------------------------------------------------ the linear filter's

def run_linear(cd, batch, w, lo, hi, u=None, bias=0, **kw):
    got = cd.filter_linear(batch, [int(v) for v in w], lo=lo, hi=hi, lag_weights=None if u is None else [int(v) for v in u], bias=bias, **kw)
    return got["mask"].cpu().numpy(), got["counts"].cpu().numpy().astype(np.int64)


def raw_linear(sz, cd, batch, codec, esz, D, chunk_len, w, u, bias, lo, hi, mask, counts, rets, tmp=None):
    """the C entry point itself, on the current stream"""
    import torch
    from sprintz_amd import _lib, rowops
    w_t, u_t, bias, lo, hi = rowops.linear_terms(w, u, bias, lo, hi, D, esz, torch.device("cuda:0"))
    if u_t is not None and tmp is None:
        tmp = torch.empty(_lib.filter_linear_tmp_bytes(esz, batch.nchunks, D) // 8, dtype=torch.int64, device="cuda")
    _lib.check(_lib.filter_linear(_lib.CODEC_DELTA if codec == "delta" else _lib.CODEC_XFF, esz, batch.data.data_ptr(), batch.offsets.data_ptr(),
                                  batch.nchunks, chunk_len, D, w_t.data_ptr(), u_t.data_ptr() if u_t is not None else None, bias, lo, hi, 0,
                                  tmp.data_ptr() if tmp is not None else None, mask.data_ptr() if mask is not None else None,
                                  counts.data_ptr() if counts is not None else None, rets.data_ptr() if rets is not None else None,
                                  C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()


# ------------------------------------------------------------------ extrema rows'

OUTS = ("min", "max", "argmin", "argmax", "first", "last", "rows", "count")       # in the order of their op bits
EXT_OPS = {k: 1 << i for i, k in enumerate(OUTS)}
ELEM = ("min", "max", "first", "last")


def run_ext(batch, codec, esz, D, chunk_len, mask, W, ops=255, byte=0x5A, general=False, mask_shift=0, null_unselected=False, stream=None):
    """the C entry point on sentinel-filled outputs of nchunks * nwin (* D, * 2) entries + PAD -> ({op: numpy incl. padding}, rets [nchunks])"""
    import torch
    from sprintz_amd import _lib
    n = batch.nchunks
    R = chunk_len // D
    nwin = -(-R // W)
    m = n * nwin
    size = {k: m * D for k in OUTS}
    size.update(rows=2 * m, count=m)
    bufs = {}
    for k in OUTS:
        if k in ELEM:
            bufs[k] = torch.from_numpy(np.full(size[k] + AGG_PAD, sentinel(esz, byte), DTYPES[esz]).view(np.int8 if esz == 1 else np.int16)).cuda()
        else:
            bufs[k] = torch.from_numpy(np.full(size[k] + AGG_PAD, sentinel(4, byte), np.uint32).view(np.int32)).cuda()
    rets_t = torch.full((n + 1,), -77, dtype=torch.int64, device="cuda")
    mask_t = None
    if mask is not None:
        flat = np.ascontiguousarray(mask, np.uint8).reshape(-1)
        mask_t = torch.from_numpy(np.concatenate([np.full(mask_shift, 0xFF, np.uint8), flat, np.full(16, 0xFF, np.uint8)])).cuda()

    def ptr(k):
        return None if null_unselected and not ops & EXT_OPS[k] else bufs[k].data_ptr()
    st = torch.cuda.current_stream() if stream is None else stream
    with torch.cuda.stream(st):
        _lib.check(_lib.extrema_rows(_lib.CODEC_DELTA if codec == "delta" else _lib.CODEC_XFF, esz, batch.data.data_ptr(), batch.offsets.data_ptr(),
                                     n, chunk_len, D, mask_t.data_ptr() + mask_shift if mask_t is not None else None, W, ops,
                                     _lib.QUERY_GENERAL_LAYOUT if general else 0, *[ptr(k) for k in OUTS], rets_t.data_ptr(),
                                     C.c_void_p(st.cuda_stream)))
    torch.cuda.synchronize()
    r = rets_t.cpu().numpy()
    assert r[n] == -77, "rets written past nchunks"
    got = {k: bufs[k].cpu().numpy().view(DTYPES[esz] if k in ELEM else np.uint32) for k in OUTS}
    return got, r[:n]


def check_ext(x, batch, codec, esz, D, chunk_len, mask, W, msg, want=None, ops=255, byte=0x5A, skip_chunk=None, **kw):
    """every selected output, the unselected ones, the padding and rets against the model; skip_chunk: a damaged chunk, whose own entries
    are unspecified"""
    want = em.extrema_rows(x, chunk_len, D, mask, W) if want is None else want
    got, rets = run_ext(batch, codec, esz, D, chunk_len, mask, W, ops, byte, **kw)
    lens = np.array(fm.chunk_counts(x.size, chunk_len))
    keep = np.arange(batch.nchunks) != (-1 if skip_chunk is None else skip_chunk)
    assert np.array_equal(rets[keep], lens[keep]), ("rets",) + msg
    if skip_chunk is not None:
        assert rets[skip_chunk] < 0, ("rets of the damaged chunk",) + msg
    for k in OUTS:
        w = want[k]
        sent = sentinel(esz if k in ELEM else 4, byte)
        g = got[k]
        assert np.all(g[w.size:] == sent), (k, "padding") + msg
        g = g[:w.size].reshape(w.shape)
        if ops & EXT_OPS[k]:
            if not np.array_equal(g[keep], w[keep]):
                bad = np.argwhere(g[keep] != w[keep])[0]
                raise AssertionError((k,) + msg + ("first difference at", tuple(bad), "got", g[keep][tuple(bad)], "want", w[keep][tuple(bad)]))
        else:
            assert np.all(g == sent), (k, "an unselected output was written") + msg
    return want


# ------------------------------------------------------------------ group-by rows'

GBY_PAD = 1024                      # entries behind d_count and behind d_sum that must keep the sentinel


def run_gby(batch, codec, esz, D, chunk_len, key, mask, key_lo, shift, nbins, H, ops=3, general=False, mask_shift=0, pass_unselected=False):
    """the C entry point on sentinel-filled d_count of ntables * nbins entries + PAD and d_sum of ntables * nbins * D + PAD; an output that
    ops does not select is NULL, or (pass_unselected) a sentinel-filled buffer that must come back untouched
    -> (count incl. padding or None, sum incl. padding or None, rets [nchunks])"""
    import torch
    from sprintz_amd import _lib
    n = batch.nchunks
    nt = -(-n // H) if H else 1
    cnt_t = torch.from_numpy(np.full(nt * nbins + GBY_PAD, SENT, np.uint64).view(np.int64)).cuda() if (ops & 1) or pass_unselected else None
    sum_t = torch.from_numpy(np.full(nt * nbins * D + GBY_PAD, SENT, np.uint64).view(np.int64)).cuda() if (ops & 2) or pass_unselected else None
    rets_t = torch.full((n + 1,), -77, dtype=torch.int64, device="cuda")
    mask_ptr = None
    if mask is not None:
        flat = np.ascontiguousarray(mask, np.uint8).reshape(-1)
        mask_t = torch.from_numpy(np.concatenate([np.full(mask_shift, 0xFF, np.uint8), flat, np.full(16, 0xFF, np.uint8)])).cuda()
        mask_ptr = mask_t.data_ptr() + mask_shift
    _lib.check(_lib.groupby_rows(_lib.CODEC_DELTA if codec == "delta" else _lib.CODEC_XFF, esz, batch.data.data_ptr(), batch.offsets.data_ptr(),
                                 n, chunk_len, D, mask_ptr, key, key_lo, shift, nbins, H, ops, _lib.QUERY_GENERAL_LAYOUT if general else 0,
                                 cnt_t.data_ptr() if cnt_t is not None else None, sum_t.data_ptr() if sum_t is not None else None,
                                 rets_t.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    r = rets_t.cpu().numpy()
    assert r[n] == -77, "rets written past nchunks"
    return (None if cnt_t is None else cnt_t.cpu().numpy().view(np.uint64), None if sum_t is None else sum_t.cpu().numpy().view(np.uint64), r[:n])


def check_gby(x, batch, codec, esz, D, chunk_len, key, mask, key_lo, shift, nbins, H, msg, want=None, skip_table=None, bad_chunk=None, ops=3, **kw):
    """d_count, d_sum, their padding and rets against the model; skip_table: a damaged chunk's table, which is unspecified"""
    want = gm.groupby_rows(x, chunk_len, D, key, mask, key_lo, shift, nbins, H) if want is None else want
    cnt, tot, rets = run_gby(batch, codec, esz, D, chunk_len, key, mask, key_lo, shift, nbins, H, ops=ops, **kw)
    lens = np.array(fm.chunk_counts(x.size, chunk_len))
    keep_c = np.arange(batch.nchunks) != (-1 if bad_chunk is None else bad_chunk)
    assert np.array_equal(rets[keep_c], lens[keep_c]), ("rets",) + msg
    if bad_chunk is not None:
        assert rets[bad_chunk] < 0, ("rets of the damaged chunk",) + msg
    keep_t = np.arange(want[0].shape[0]) != (-1 if skip_table is None else skip_table)
    for name, got, w, bit in (("count", cnt, want[0], 1), ("sum", tot, want[1], 2)):
        if ops & bit:
            assert np.all(got[w.size:] == SENT), (name, "padding") + msg
            assert np.array_equal(got[:w.size].reshape(w.shape)[keep_t], w[keep_t]), (name,) + msg
        elif got is not None:
            assert np.all(got == SENT), (name, "not selected, and written") + msg
    return want


# ------------------------------------------------------------------ moments rows'

MOM_OPS = {"count": 1, "sum": 2, "sumsq": 4, "cross": 8}


def run_mom(batch, codec, esz, D, chunk_len, mask, W, ref, ops=15, byte=0x5A, general=False, mask_shift=0, null_unselected=False):
    """the C entry point on sentinel-filled outputs of nchunks * nwin (* D) entries + PAD -> ({op: numpy incl. padding}, rets [nchunks]);
    mask None: a NULL d_mask"""
    import torch
    from sprintz_amd import _lib
    n = batch.nchunks
    R = chunk_len // D
    nwin = -(-R // W)
    m = n * nwin
    bufs = {k: torch.from_numpy(np.full(m * D + AGG_PAD, sentinel(8, byte), np.uint64).view(np.int64)).cuda() for k in ("sum", "sumsq", "cross")}
    bufs["count"] = torch.from_numpy(np.full(m + AGG_PAD, sentinel(4, byte), np.uint32).view(np.int32)).cuda()
    rets_t = torch.full((n + 1,), -77, dtype=torch.int64, device="cuda")
    mask_ptr = None
    if mask is not None:
        flat = np.ascontiguousarray(mask, np.uint8).reshape(-1)
        mask_t = torch.from_numpy(np.concatenate([np.full(mask_shift, 0xFF, np.uint8), flat, np.full(16, 0xFF, np.uint8)])).cuda()
        mask_ptr = mask_t.data_ptr() + mask_shift

    def ptr(k):
        return None if null_unselected and not ops & MOM_OPS[k] else bufs[k].data_ptr()
    _lib.check(_lib.moments_rows(_lib.CODEC_DELTA if codec == "delta" else _lib.CODEC_XFF, esz, batch.data.data_ptr(), batch.offsets.data_ptr(),
                                 n, chunk_len, D, mask_ptr, W, ops, ref, _lib.QUERY_GENERAL_LAYOUT if general else 0,
                                 ptr("count"), ptr("sum"), ptr("sumsq"), ptr("cross"), rets_t.data_ptr(),
                                 C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    r = rets_t.cpu().numpy()
    assert r[n] == -77, "rets written past nchunks"
    got = {k: bufs[k].cpu().numpy().view(np.uint64) for k in ("sum", "sumsq", "cross")}
    got["count"] = bufs["count"].cpu().numpy().view(np.uint32)
    return got, r[:n]


def check_mom(x, batch, codec, esz, D, chunk_len, mask, W, ref, msg, want=None, ops=15, byte=0x5A, skip_chunk=None, **kw):
    """every selected output, the unselected ones, the padding and rets against the model; skip_chunk: a damaged chunk, whose own entries
    are unspecified"""
    want = mm.moments_rows(x, chunk_len, D, mask, W, ref) if want is None else want
    got, rets = run_mom(batch, codec, esz, D, chunk_len, mask, W, ref, ops, byte, **kw)
    lens = np.array(fm.chunk_counts(x.size, chunk_len))
    keep = np.arange(batch.nchunks) != (-1 if skip_chunk is None else skip_chunk)
    assert np.array_equal(rets[keep], lens[keep]), ("rets",) + msg
    if skip_chunk is not None:
        assert rets[skip_chunk] < 0, ("rets of the damaged chunk",) + msg
    for k in ("count", "sum", "sumsq", "cross"):
        w = want[k]
        sent = sentinel(4 if k == "count" else 8, byte)
        g = got[k]
        assert np.all(g[w.size:] == sent), (k, "padding") + msg
        g = g[:w.size].reshape(w.shape)
        if ops & MOM_OPS[k]:
            assert np.array_equal(g[keep], w[keep]), (k,) + msg
        else:
            assert np.all(g == sent), (k, "an unselected output was written") + msg
    return want


# ------------------------------------------------------------------ zone maps'

def host(t):
    import torch
    if t.dtype == torch.uint16:
        return t.view(torch.int16).cpu().numpy().view(np.uint16)
    return t.cpu().numpy()


def assert_zone_map(z, x, chunk_len, D, esz, msg):
    zmin, zmax, zlen = zm.zone_map(x, chunk_len, D, esz)
    assert np.array_equal(host(z.len), zlen), ("zlen",) + msg
    assert np.array_equal(host(z.min), zmin) and np.array_equal(host(z.max), zmax), ("zone",) + msg
    return zmin, zmax, zlen
