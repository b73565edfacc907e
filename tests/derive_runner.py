"""What the two tiers of derive rows' tests share: the refusals of the C entry point, as one list for host and device pointers, and the GPU
tier's launch on sentinel-filled buffers with its comparison (tests/test_gpu_project.py's run_project / assert_project, for this mode)."""
import ctypes as C

import numpy as np

import derive_model as dm
from fixtures import refusals

PAD = 1024                                             # sentinel elements in front of and behind the output
SENT = {2: 0x5A5A, 4: 0x5A5A5A5A}
CODEC_ID = {"delta": 0, "xff": 1}


def good_args(p):
    """a call that passes every check, on 16384 bytes at the 16-byte aligned address p"""
    return dict(codec=1, esz=2, comp=p, offs=p, n=3, cl=8 * 67, D=8, K=2, w=p + 1024, u=None, bias=None, fmt=0, scale=None, offset=None, prev=None,
                flags=0, tmp=None, out=p + 4096, rets=p + 12288)


def derive_call(lib, p):
    good = good_args(p)

    def call(**kw):
        a = dict(good, **kw)
        return lib.derive_rows(a["codec"], a["esz"], a["comp"], a["offs"], a["n"], a["cl"], a["D"], a["K"], a["w"], a["u"], a["bias"], a["fmt"], a["scale"],
                               a["offset"], a["prev"], a["flags"], a["tmp"], a["out"], a["rets"], None)
    return call


def check_refusals(lib, p):
    """every refusal the header lists, each with its code and a message that names derive_rows; then the calls that return 0 without a launch"""
    call = derive_call(lib, p)
    invalid, unsupported = refusals(lib, call, "derive_rows")
    invalid(K=0)
    invalid(K=17)
    invalid(cl=8 * 67 + 1)                                                       # chunk_len % ndims != 0
    invalid(D=7)
    invalid(cl=0)
    invalid(flags=2)                                                             # unknown flags
    invalid(flags=4)
    invalid(scale=p + 2048)                                                      # scale / offset with the int32 format
    invalid(offset=p + 2048)
    for fmt in (-1, 4, 7):
        invalid(fmt=fmt)
    for k in ("comp", "offs", "w", "out"):
        invalid(**{k: None})
    invalid(out=p + 4098)                                                        # misaligned to the output element: 4 bytes as int32 and float32, 2 as a 16-bit float
    invalid(fmt=1, out=p + 4098)
    invalid(fmt=2, out=p + 4097)
    invalid(w=p + 1026)
    invalid(u=p + 2050, tmp=p + 8192)
    invalid(bias=p + 2049)
    invalid(fmt=1, scale=p + 2050)
    invalid(fmt=3, offset=p + 2049)
    invalid(prev=p + 3073)                                                       # to the element size
    invalid(rets=p + 12292)
    invalid(u=p + 2048)                                                          # a lag term without its scratch
    invalid(u=p + 2048, tmp=p + 8196)                                            # ... or with a misaligned one
    assert call(D=0) == lib.E_INVALID and call(codec=9) == lib.E_INVALID and call(esz=3) == lib.E_INVALID
    unsupported(D=513, cl=513 * 64)                                              # more than 512 columns
    for codec in (2, 3):
        unsupported(codec=codec)                                                 # the non-RLE codecs
    assert call(n=0) == 0 and call(n=0, u=p + 2048, tmp=p + 8192, prev=p + 3072) == 0      # nothing to do: returns 0, launches nothing
    return call


def run_derive(batch, codec, esz, D, chunk_len, w, u=None, bias=None, fmt=dm.I32, scale=None, offset=None, prev=None, general=False, shift=0):
    """the C entry point on sentinel-filled buffers: the output has PAD + shift elements in front, nchunks x R x K of its own -- a chunk slot each
    chunk -- and PAD behind; rets one entry behind; the scratch starts dirty.  w, u: int [K, D]; bias: int [K] or None; prev: [D] of the element
    type or None.  -> (the whole output buffer as bits, rets [nchunks + 1])"""
    import torch
    from sprintz_amd import _lib
    nch = batch.nchunks
    w = np.ascontiguousarray(np.asarray(w, np.int64).reshape(-1, D).astype(np.int32))
    K = w.shape[0]
    osz = dm.OUT_BYTES[fmt]
    dt = {2: torch.int16, 4: torch.int32}[osz]
    buf = torch.full((PAD + shift + nch * (chunk_len // D) * K + PAD,), SENT[osz], dtype=dt, device="cuda")
    rets = torch.full((nch + 1,), -77, dtype=torch.int64, device="cuda")
    dev = lambda a, t: None if a is None else torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(t))).cuda()      # noqa: E731
    w_t, u_t, b_t = dev(w, np.int32), dev(None if u is None else np.asarray(u, np.int64).reshape(K, D), np.int32), dev(bias, np.int32)
    sc, of = dev(scale, np.float32), dev(offset, np.float32)
    pv = None if prev is None else torch.from_numpy(np.ascontiguousarray(prev).view(np.int8 if esz == 1 else np.int16)).cuda()
    tmp = torch.full((max(_lib.derive_rows_tmp_bytes(esz, nch, D), 8),), 0x5A, dtype=torch.uint8, device="cuda") if u is not None else None
    ptr = lambda t: None if t is None else t.data_ptr()      # noqa: E731
    _lib.check(_lib.derive_rows(CODEC_ID[codec], esz, batch.data.data_ptr(), batch.offsets.data_ptr(), nch, chunk_len, D, K, ptr(w_t), ptr(u_t), ptr(b_t),
                                dm.C_FORMAT[fmt], ptr(sc), ptr(of), ptr(pv), _lib.QUERY_GENERAL_LAYOUT if general else 0, ptr(tmp),
                                buf.data_ptr() + (PAD + shift) * osz, rets.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    return buf.cpu().numpy().view({2: np.uint16, 4: np.uint32}[osz]), rets.cpu().numpy()


def assert_derive(buf, rets, n, chunk_len, nchunks, D, K, want, shift, msg, bad=(), lag=False):
    """the output against `want` [G, K], G = n // D whole rows -- outside the chunks in `bad` and, with a lag term, outside row 0 of the chunk behind
    each of them: one row a damaged chunk -- and the sentinel everywhere else: in front, behind, and at the K places of a partial last row; rets are
    the chunks' element counts (negative for the chunks in `bad`), with the sentinel behind"""
    G, R = n // D, chunk_len // D
    sent = SENT[buf.dtype.itemsize]
    assert buf.size == PAD + shift + nchunks * R * K + PAD, (buf.size,) + msg
    assert np.all(buf[:PAD + shift] == sent), ("written in front",) + msg
    assert np.all(buf[PAD + shift + G * K:] == sent), ("written behind the batch's last whole row",) + msg
    body = buf[PAD + shift:PAD + shift + G * K].reshape(G, K)
    assert want.shape == (G, K) and want.dtype == body.dtype, (want.shape, want.dtype, body.dtype) + msg
    keep = np.ones((G, K), bool)
    for c in bad:
        keep[c * R:(c + 1) * R] = False
        if lag:
            keep[(c + 1) * R:(c + 1) * R + 1] = False
    assert int((~keep).all(axis=1).sum()) <= len(bad) * (R + (1 if lag else 0))
    ne = (body != want) & keep
    assert not ne.any(), (int(ne.sum()), "of", int(keep.sum()), "values differ; first at", tuple(int(v) for v in np.argwhere(ne)[0]),
                          [hex(int(v)) for v in (body[ne][0], want[ne][0])]) + msg
    lens = [min(chunk_len, n - c * chunk_len) for c in range(nchunks)]
    assert all(rets[c] == lens[c] for c in range(nchunks) if c not in bad) and all(rets[c] < 0 for c in bad) and rets[nchunks] == -77, ("rets", rets.tolist()) + msg
