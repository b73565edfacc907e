"""What the two tiers of FIR rows' tests share: the refusals of the C entry point, as one list for host and device pointers, and the GPU tier's
launch on sentinel-filled buffers with its comparison (tests/derive_runner.py's run_derive / assert_derive, for this mode)."""
import ctypes as C

import numpy as np

import fir_model as fm
from fixtures import refusals

PAD = 1024                                             # sentinel elements in front of and behind the output; sentinel bytes around the scratch
SENT = {2: 0x5A5A, 4: 0x5A5A5A5A}
CODEC_ID = {"delta": 0, "xff": 1}


def good_args(p):
    """a call that passes every check, on 16384 bytes at the 16-byte aligned address p"""
    return dict(codec=1, esz=2, comp=p, offs=p, n=3, cl=8 * 67, D=8, T=9, taps=p + 1024, bias=None, fmt=0, scale=None, offset=None, prev=None,
                flags=0, tmp=p + 8192, out=p + 4096, rets=p + 12288)


def fir_call(lib, p):
    good = good_args(p)

    def call(**kw):
        a = dict(good, **kw)
        return lib.fir_rows(a["codec"], a["esz"], a["comp"], a["offs"], a["n"], a["cl"], a["D"], a["T"], a["taps"], a["bias"], a["fmt"], a["scale"],
                            a["offset"], a["prev"], a["flags"], a["tmp"], a["out"], a["rets"], None)
    return call


def check_refusals(lib, p):
    """every refusal the header lists, each with its code and a message that names fir_rows; then the calls that return 0 without a launch"""
    call = fir_call(lib, p)
    invalid, unsupported = refusals(lib, call, "fir_rows")
    invalid(T=0)
    invalid(T=257)
    invalid(T=69)                                                                # ntaps - 1 > chunk_len / ndims = 67
    invalid(cl=8 * 67 + 1)                                                       # chunk_len % ndims != 0
    invalid(D=7)
    invalid(cl=0)
    invalid(flags=2)                                                             # unknown flags
    invalid(flags=4)
    invalid(scale=p + 2048)                                                      # scale / offset with the int32 format
    invalid(offset=p + 2048)
    for fmt in (-1, 4, 7):
        invalid(fmt=fmt)
    for k in ("comp", "offs", "taps", "out"):
        invalid(**{k: None})
    invalid(out=p + 4098)                                                        # misaligned to the output element: 4 bytes as int32 and float32, 2 as a 16-bit float
    invalid(fmt=1, out=p + 4098)
    invalid(fmt=2, out=p + 4097)
    invalid(taps=p + 1026)
    invalid(bias=p + 2049)
    invalid(fmt=1, scale=p + 2050)
    invalid(fmt=3, offset=p + 2049)
    invalid(prev=p + 3073)                                                       # to the element size
    assert call(n=0, T=1, tmp=None, prev=p + 3073) == 0                          # ... but ignored, whatever it is, with one tap
    invalid(rets=p + 12292)
    invalid(tmp=None)                                                            # more than one tap without its scratch
    invalid(tmp=p + 8200)                                                        # ... or with a misaligned one
    assert call(D=0) == lib.E_INVALID and call(codec=9) == lib.E_INVALID and call(esz=3) == lib.E_INVALID
    unsupported(D=513, cl=513 * 64)                                              # more than 512 columns
    for codec in (2, 3):
        unsupported(codec=codec)                                                 # the non-RLE codecs
    # a history that fits no workgroup's LDS for the shape: the message names the largest ntaps the shape takes
    for esz, D, general in ((2, 512, 0), (1, 300, 0), (2, 300, 0)):
        tmax = fm.max_taps(esz, D, general)
        if tmax < fm.MAX_TAPS:
            unsupported(esz=esz, D=D, cl=D * 400, T=tmax + 1)
            assert f"the largest ntaps allowed is {tmax}" in lib.last_error(), lib.last_error()
    assert fm.max_taps(2, 512, 0) < fm.MAX_TAPS                                  # (so that the loop above met the refusal)
    assert call(n=0) == 0 and call(n=0, T=1, tmp=None) == 0 and call(n=0, prev=p + 3072) == 0      # nothing to do: returns 0, launches nothing
    return call


def run_fir(batch, codec, esz, D, chunk_len, taps, bias=None, fmt=fm.I32, scale=None, offset=None, prev=None, general=False, shift=0):
    """the C entry point on sentinel-filled buffers: the output has PAD + shift elements in front, nchunks x chunk_len of its own -- a chunk slot
    each chunk -- and PAD behind; rets one entry behind; the scratch starts dirty, with PAD sentinel bytes on either side.  taps: int [T, D];
    bias: int [D] or None; prev: [T - 1, D] of the element type or None.  -> (the whole output buffer as bits, rets [nchunks + 1])"""
    import torch
    from sprintz_amd import _lib
    nch = batch.nchunks
    taps = np.ascontiguousarray(np.asarray(taps, np.int64).reshape(-1, D).astype(np.int32))
    T = taps.shape[0]
    osz = fm.OUT_BYTES[fmt]
    dt = {2: torch.int16, 4: torch.int32}[osz]
    buf = torch.full((PAD + shift + nch * chunk_len + PAD,), SENT[osz], dtype=dt, device="cuda")
    rets = torch.full((nch + 1,), -77, dtype=torch.int64, device="cuda")
    dev = lambda a, t: None if a is None else torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(t))).cuda()      # noqa: E731
    t_t, b_t, sc, of = dev(taps, np.int32), dev(bias, np.int32), dev(scale, np.float32), dev(offset, np.float32)
    pv = None if prev is None or T == 1 else torch.from_numpy(np.ascontiguousarray(prev).reshape(-1).view(np.int8 if esz == 1 else np.int16)).cuda()
    nb = int(_lib.fir_rows_tmp_bytes(esz, nch, D, T))
    assert nb == (nch * fm.tmp_stride(T, D, esz) if T > 1 else 0)
    tmp = torch.full((PAD + nb + PAD,), 0x5A, dtype=torch.uint8, device="cuda") if T > 1 else None
    assert tmp is None or (tmp.data_ptr() + PAD) % 16 == 0
    ptr = lambda t: None if t is None else t.data_ptr()      # noqa: E731
    _lib.check(_lib.fir_rows(CODEC_ID[codec], esz, batch.data.data_ptr(), batch.offsets.data_ptr(), nch, chunk_len, D, T, ptr(t_t), ptr(b_t),
                             fm.C_FORMAT[fmt], ptr(sc), ptr(of), ptr(pv), _lib.QUERY_GENERAL_LAYOUT if general else 0,
                             None if tmp is None else tmp.data_ptr() + PAD, buf.data_ptr() + (PAD + shift) * osz, rets.data_ptr(),
                             C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    if tmp is not None:
        t_np = tmp.cpu().numpy()
        assert np.all(t_np[:PAD] == 0x5A) and np.all(t_np[PAD + nb:] == 0x5A), "written outside the scratch"
    return buf.cpu().numpy().view({2: np.uint16, 4: np.uint32}[osz]), rets.cpu().numpy()


def assert_fir(buf, rets, n, chunk_len, nchunks, D, T, want, shift, msg, bad=()):
    """the output against `want` [n] -- outside the chunks in `bad` and outside the first T - 1 rows of the chunk behind each of them -- and the
    sentinel everywhere else: in front, behind, and at the elements that do not exist; rets are the chunks' element counts (negative for the chunks
    in `bad`), with the sentinel behind"""
    sent = SENT[buf.dtype.itemsize]
    assert buf.size == PAD + shift + nchunks * chunk_len + PAD, (buf.size,) + msg
    assert np.all(buf[:PAD + shift] == sent), ("written in front",) + msg
    assert np.all(buf[PAD + shift + n:] == sent), ("written behind the batch's last element",) + msg
    body = buf[PAD + shift:PAD + shift + n]
    assert want.shape == (n,) and want.dtype == body.dtype, (want.shape, want.dtype, body.dtype) + msg
    keep = np.ones(n, bool)
    for c in bad:
        keep[c * chunk_len:(c + 1) * chunk_len] = False
        keep[(c + 1) * chunk_len:(c + 1) * chunk_len + (T - 1) * D] = False
    ne = (body != want) & keep
    assert not ne.any(), (int(ne.sum()), "of", int(keep.sum()), "values differ; first at element", int(np.argwhere(ne)[0][0]), "row in chunk",
                          int(np.argwhere(ne)[0][0]) % chunk_len // D, [hex(int(v)) for v in (body[ne][0], want[ne][0])]) + msg
    lens = [min(chunk_len, n - c * chunk_len) for c in range(nchunks)]
    assert all(rets[c] == lens[c] for c in range(nchunks) if c not in bad) and all(rets[c] < 0 for c in bad) and rets[nchunks] == -77, ("rets", rets.tolist()) + msg
