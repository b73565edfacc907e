"""What the GPU tests of cumulative rows share: the C entry point on sentinel-filled buffers with guard bands, the comparison with the model
(tests/cumulative_model.py), and the launches a call must make according to the planner."""
import ctypes as C
from types import SimpleNamespace

import numpy as np

import cumulative_model as cm

PAD = 1024                                             # sentinel elements in front of and behind every output
TPAD = 256                                             # sentinel bytes in front of and behind the scratch and the carry
BYTE = 0xA5
CODEC_ID = {"delta": 0, "xff": 1}
Q_WINDOW, Q_CUMULATIVE = 3, 17
RETS_SENT = -77
NP_OUT = {1: np.uint8, 2: np.uint16, 4: np.int32, 8: np.int64}


def sent(dtype):
    """0xA5 repeated over an element of `dtype`"""
    return np.frombuffer(bytes([BYTE]) * np.dtype(dtype).itemsize, dtype)[0]


def out_bytes(name, esz, sb):
    return sb if name == "sum" else esz


def launches(plan, codec, esz, D, chunk_len, nchunks, ops, sb, general=False, no_fast=0, cpg=1, out_lo=0):
    """-> (the decode launch's family, {family: launches} of the whole call): with more than one chunk the totals pass -- the windowed query,
    wherever the planner sends it -- and the decode; the scan is no decoder family"""
    common = dict(esz=esz, D=D, chunk_len=chunk_len, nchunks=nchunks, codec=CODEC_ID[codec], general=general, no_fast=no_fast, chunks_per_group=cpg)
    dec = plan(q=Q_CUMULATIVE, out_esz=cm.out_esz(esz, ops, sb), out_lo=out_lo, **common)["family"]
    assert dec in ("dec_fast", "dec_generic"), dec
    counts = {dec: 1}
    if nchunks > 1:
        tot = plan(q=Q_WINDOW, **common)["family"]
        counts[tot] = counts.get(tot, 0) + 1
    return dec, counts


def run(batch, codec, esz, D, chunk_len, ops=7, sb=8, carry=None, general=False, shift=0, with_tmp=True, with_carry_out=True, stream=None, bufs=None):
    """the C entry point on 0xA5-filled buffers: each selected output has PAD + shift elements in front, nchunks * chunk_len of its own and
    PAD behind, an unselected one is NULL; the scratch and carry_out have TPAD bytes around them; rets one entry behind.  carry: uint64
    [3, D] or None.  bufs: the buffers of an earlier call, used again as they are (dirty).
    -> outs {op: the whole buffer}, rets [nchunks + 1], carry uint64 [3, D] or None, bufs"""
    import torch
    from sprintz_amd import _lib
    n = batch.nchunks
    tbytes = cm.tmp_bytes(n, D)
    if bufs is None:
        bufs = {}
        for name in cm.names(ops):
            osz = out_bytes(name, esz, sb)
            bufs[name] = torch.full(((PAD + shift + n * chunk_len + PAD) * osz,), BYTE, dtype=torch.uint8, device="cuda")
        bufs["tmp"] = torch.full((TPAD + tbytes + TPAD,), BYTE, dtype=torch.uint8, device="cuda")
        bufs["cout"] = torch.full((TPAD + 24 * D + TPAD,), BYTE, dtype=torch.uint8, device="cuda")
        bufs["rets"] = torch.full((n + 1,), RETS_SENT, dtype=torch.int64, device="cuda")
    ptrs = {name: (bufs[name].data_ptr() + (PAD + shift) * out_bytes(name, esz, sb) if name in bufs else None) for name in ("min", "max", "sum")}
    cin = None if carry is None else torch.from_numpy(np.ascontiguousarray(carry, dtype=np.uint64).view(np.int64)).cuda()
    st = torch.cuda.current_stream() if stream is None else stream
    with torch.cuda.stream(st):
        _lib.check(_lib.cumulative_rows(CODEC_ID[codec], esz, batch.data.data_ptr(), batch.offsets.data_ptr(), n, chunk_len, D, ops, sb,
                                        _lib.QUERY_GENERAL_LAYOUT if general else 0, ptrs["min"], ptrs["max"], ptrs["sum"],
                                        None if cin is None else cin.data_ptr(), bufs["cout"].data_ptr() + TPAD if with_carry_out else None,
                                        bufs["tmp"].data_ptr() + TPAD if with_tmp else None, bufs["rets"].data_ptr(), C.c_void_p(st.cuda_stream)))
    torch.cuda.synchronize()
    t = bufs["tmp"].cpu().numpy()
    assert np.all(t[:TPAD] == BYTE) and np.all(t[TPAD + tbytes:] == BYTE), "written around the scratch"
    if not with_tmp:
        assert np.all(t == BYTE), "the scratch was not given"
    c = bufs["cout"].cpu().numpy()
    assert np.all(c[:TPAD] == BYTE) and np.all(c[TPAD + 24 * D:] == BYTE), "written around carry_out"
    left = c[TPAD:TPAD + 24 * D].view(np.uint64).reshape(3, D).copy() if with_carry_out else None
    if not with_carry_out:
        assert np.all(c == BYTE), "carry_out was not given"
    outs = {name: bufs[name].cpu().numpy().view(NP_OUT[out_bytes(name, esz, sb)] if name == "sum" else NP_OUT[esz]) for name in cm.names(ops)}
    return SimpleNamespace(outs=outs, rets=bufs["rets"].cpu().numpy(), carry=left, bufs=bufs)


def want_of(x, D, ops, sb, carry=None, chunk_len=None, bad=()):
    """the model's outputs in the library's forms, and its carry"""
    got, left = cm.cumulative(x, D, carry, ops, chunk_len, bad)
    if "sum" in got:
        got["sum"] = cm.int64(got["sum"]) if sb == 8 else cm.low32(got["sum"])
    return got, left


def check(res, x, chunk_len, nchunks, D, ops, sb, msg, carry=None, shift=0, bad=()):
    """every selected output against the model, exactly: the chunks outside `bad` are the model's with the bad chunks absent; nothing is
    written in front, behind, or past the short last chunk's count; rets are the chunks' element counts (negative in `bad`), with the
    sentinel behind; carry_out (where it was asked for) is the model's"""
    n, ne = x.size, nchunks * chunk_len
    want, left = want_of(x, D, ops, sb, carry, chunk_len, bad)
    assert set(res.outs) == set(cm.names(ops)), (sorted(res.outs),) + msg
    keep = np.ones(n, bool)
    for c in bad:
        keep[c * chunk_len:(c + 1) * chunk_len] = False
    for name, buf in res.outs.items():
        s = sent(buf.dtype)
        assert buf.size == PAD + shift + ne + PAD
        assert np.all(buf[:PAD + shift] == s), (name, "written in front") + msg
        assert np.all(buf[PAD + shift + ne:] == s), (name, "written behind") + msg
        body = buf[PAD + shift:PAD + shift + ne]
        assert np.all(body[n:] == s), (name, "written past the last chunk's count") + msg
        diff = body[:n][keep] != want[name][keep]
        assert not diff.any(), (name, int(diff.sum()), "of", int(keep.sum()), "elements differ; first at", int(np.flatnonzero(keep)[np.flatnonzero(diff)[0]])) + msg
    lens = [min(chunk_len, n - c * chunk_len) for c in range(nchunks)]
    assert all(res.rets[c] == lens[c] for c in range(nchunks) if c not in bad) and all(res.rets[c] < 0 for c in bad) and res.rets[nchunks] == RETS_SENT, \
        ("rets", res.rets.tolist()) + msg
    if res.carry is not None:
        assert np.array_equal(res.carry, left), ("carry_out", res.carry.tolist(), left.tolist()) + msg
    return want, left


def random_carry(rng, D, esz):
    """seeds that matter: minima and maxima inside the type's range, sums anywhere in 64 bits"""
    top = 1 << (8 * esz)
    return np.stack([rng.integers(top // 2, top, D).astype(np.uint64), rng.integers(0, top // 2, D).astype(np.uint64), rng.integers(0, 1 << 64, D, dtype=np.uint64)])
