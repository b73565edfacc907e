"""Host-side mirror of the reference interface for the codec path.

Two layers, both thin over the C-ABI (include/sprintz_mi355x.h):

* ``sprintz_compress_delta_8b(src, len, dest, ndims, write_size=True)`` & co:
  the eight functions of the reference's cpp/Compress/sprintz.h:16-32 with the
  same names, argument order, units (ELEMENTS) and return values; ``src`` and
  ``dest`` are caller-owned numpy arrays, as the reference's are caller-owned
  C buffers.  One call == one chunk on the GPU: correct, not fast.

* ``ChunkedCodec``: the batched device API on torch tensors resident in HBM;
  this is what bench.py measures.  Chunk == independent compress() call
  (lzbench block, reference README.md:58).
"""
import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib, rowops

_NP = {1: np.uint8, 2: np.uint16}
_CODEC_ID = {"delta": _lib.CODEC_DELTA, "xff": _lib.CODEC_XFF,
             "delta_norle": _lib.CODEC_DELTA_NORLE, "bitpack": _lib.CODEC_BITPACK_NORLE,    # sprintz_delta.cpp:64-1391
             "xff_norle": _lib.CODEC_XFF_NORLE}                                             # sprintz_xff.cpp:35-626, 8-bit only


def _ptr(t):
    """a tensor's device address, or NULL for None"""
    return t.data_ptr() if t is not None else None


def _np_ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _compress(codec, esz, src, length, dest, ndims, write_size):
    src = np.ascontiguousarray(src)
    if src.dtype.itemsize != esz or src.size < length:
        raise ValueError("src dtype/size does not match the call")
    if not dest.flags["C_CONTIGUOUS"] or not dest.flags["WRITEABLE"]:
        raise ValueError("dest must be a writable contiguous array")
    need = _lib.compress_bound(esz, length, ndims) if ndims else 8
    if dest.nbytes < min(need, (length * 3 // 2 + 64) * esz):
        raise ValueError("dest too small (reference callers allocate len*3/2+64 elements)")
    return int(_lib.compress[(codec, esz)](_np_ptr(src), length, _np_ptr(dest), ndims, int(bool(write_size))))


def _decompress(codec, esz, src, dest):
    src = np.ascontiguousarray(src)
    if not dest.flags["C_CONTIGUOUS"] or not dest.flags["WRITEABLE"]:
        raise ValueError("dest must be a writable contiguous array")
    return int(_lib.decompress[(codec, esz)](_np_ptr(src), _np_ptr(dest)))


# ---- the reference's eight entry points (sprintz.h:16-32)
def sprintz_compress_delta_8b(src, len, dest, ndims, write_size=True):  # noqa: A002 - reference's name
    return _compress("delta", 1, src, len, dest, ndims, write_size)


def sprintz_decompress_delta_8b(src, dest):
    return _decompress("delta", 1, src, dest)


def sprintz_compress_xff_8b(src, len, dest, ndims, write_size=True):  # noqa: A002
    return _compress("xff", 1, src, len, dest, ndims, write_size)


def sprintz_decompress_xff_8b(src, dest):
    return _decompress("xff", 1, src, dest)


def sprintz_compress_delta_16b(src, len, dest, ndims, write_size=True):  # noqa: A002
    return _compress("delta", 2, src, len, dest, ndims, write_size)


def sprintz_decompress_delta_16b(src, dest):
    return _decompress("delta", 2, src, dest)


def sprintz_compress_xff_16b(src, len, dest, ndims, write_size=True):  # noqa: A002
    return _compress("xff", 2, src, len, dest, ndims, write_size)


def sprintz_decompress_xff_16b(src, dest):
    return _decompress("xff", 2, src, dest)


def decompress_noheader(codec, esz, src, dest, ndims, ngroups, remaining_len):
    """5-argument kernel form for write_size=False streams (sprintz_xff.h:56-58)."""
    src = np.ascontiguousarray(src)
    return int(_lib.decompress_noheader(_CODEC_ID[codec], esz, _np_ptr(src), _np_ptr(dest), ndims, ngroups, remaining_len))


# ---- batched device API ------------------------------------------------------

@dataclass
class CompressedBatch:
    """Dense container: chunk c's stream is data[offsets[c]:offsets[c]+sizes[c]]
    (each stream bit-exact with the reference's output for that chunk)."""
    data: "torch.Tensor"       # uint8, device; readable READ_SLACK bytes past total
    offsets: "torch.Tensor"    # int64 [nchunks+1], device (offsets[-1] = total bytes incl. alignment padding)
    sizes: "torch.Tensor"      # int32 [nchunks], device: exact stream bytes
    nchunks: int
    total_len: int             # elements before compression
    chunk_len: int
    ndims: int

    def total_bytes(self):
        return int(self.offsets[-1].item())

    def stream_bytes(self):
        return int(self.sizes.to("cpu", dtype=__import__("torch").int64).sum().item())


@dataclass
class ZoneMap:
    """A batch's zone map (ChunkedCodec.zone_map): every chunk's per-column minimum and maximum and its element count.  It describes the
    container as it was when the map was built, under the layout flag and the SPRINTZ_OPT_REF_DECODER_QUIRK state recorded here."""
    min: "torch.Tensor"        # codec dtype [nchunks, ndims], device  # noqa: A003
    max: "torch.Tensor"        # codec dtype [nchunks, ndims], device  # noqa: A003
    len: "torch.Tensor"        # int64 [nchunks], device: elements, or < 0 for a damaged chunk  # noqa: A003
    general_layout: bool
    quirk: int


class ChunkedCodec:
    """Batched Sprintz codec on one GPU.

    codec: "delta" | "xff"; elem_bytes: 1 | 2; ndims: columns; chunk_len:
    elements per independent chunk (10 KB of uint16 = 5120).
    """

    def __init__(self, codec, elem_bytes, ndims, chunk_len, device=None, align=16):
        import torch
        if codec not in _CODEC_ID:
            raise ValueError("codec must be 'delta', 'xff', 'delta_norle', 'bitpack' or 'xff_norle'")
        if elem_bytes not in (1, 2):
            raise ValueError("elem_bytes must be 1 or 2")
        if not torch.cuda.is_available():
            raise _lib.SprintzError(_lib.E_NO_DEVICE, "no HIP device visible to torch; there is no CPU fallback")
        self.torch = torch
        self.codec, self.esz, self.ndims, self.chunk_len, self.align = codec, elem_bytes, int(ndims), int(chunk_len), align
        dev = torch.device(device if device is not None else "cuda")
        if dev.type != "cuda":
            raise ValueError("device must be a cuda (HIP) device")
        # always an indexed device: "cuda" alone would never compare equal to a tensor's device
        self.device = torch.device("cuda", torch.cuda.current_device() if dev.index is None else dev.index)
        self.dtype = torch.uint8 if elem_bytes == 1 else torch.uint16
        self.slot_stride = int(_lib.compress_bound(elem_bytes, self.chunk_len, self.ndims))
        self._ws = {}
        self.last_prune = None             # what the last filter call with zones= pruned (filter_rows)

    def _stream(self):
        return C.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)

    def _on(self):
        """the C library launches on the CURRENT HIP device: make it this codec's for the call"""
        return self.torch.cuda.device(self.device)

    def workspace(self, nchunks):
        """slot buffer / sizes / scan scratch, cached per nchunks"""
        t = self.torch
        ws = self._ws.get(nchunks)
        if ws is None:
            ws = dict(
                slots=t.empty(nchunks * self.slot_stride, dtype=t.uint8, device=self.device),
                sizes=t.empty(nchunks, dtype=t.int32, device=self.device),
                rets=t.empty(nchunks, dtype=t.int64, device=self.device),
                tmp=t.empty(int(_lib.compress_dense_tmp_bytes(nchunks)), dtype=t.uint8, device=self.device),
            )
            self._ws = {nchunks: ws}
        return ws

    def _padded_view(self, src):
        """device tensor readable READ_SLACK bytes past its end (copy only if needed)"""
        t = self.torch
        flat = src.reshape(-1)
        buf = t.empty(flat.numel() * self.esz + _lib.READ_SLACK, dtype=t.uint8, device=self.device)
        buf[:flat.numel() * self.esz] = flat.view(t.uint8)
        return buf

    def compress_to_slots(self, src_padded_u8, total_len, ws=None):
        """encode kernel only: src (uint8 view, padded) -> slot-strided streams + sizes"""
        nchunks = int(_lib.num_chunks(total_len, self.chunk_len))
        ws = ws or self.workspace(nchunks)
        with self._on():
            _lib.check(_lib.compress_batch(_CODEC_ID[self.codec], self.esz, src_padded_u8.data_ptr(), total_len,
                                           self.chunk_len, self.ndims, ws["slots"].data_ptr(), self.slot_stride,
                                           ws["sizes"].data_ptr(), ws["rets"].data_ptr(), self._stream()))
        return ws

    def _new_container(self, nchunks, dense=None, offsets=None):
        """the dense container of nchunks chunks at their bound, readable READ_SLACK bytes past it, and its offsets (what the caller
        brought stays)"""
        t = self.torch
        if dense is None:
            dense = t.empty(nchunks * self.slot_stride + _lib.READ_SLACK, dtype=t.uint8, device=self.device)
        if offsets is None:
            offsets = t.empty(nchunks + 1, dtype=t.int64, device=self.device)
        return dense, offsets

    def compact(self, ws, nchunks, dense=None, offsets=None):
        dense, offsets = self._new_container(nchunks, dense, offsets)
        with self._on():
            _lib.check(_lib.compact(ws["slots"].data_ptr(), self.slot_stride, ws["sizes"].data_ptr(), nchunks, self.align,
                                    dense.data_ptr(), offsets.data_ptr(), ws["tmp"].data_ptr(), self._stream()))
        return dense, offsets

    def compress_dense(self, src_padded_u8, total_len, ws=None, dense=None, offsets=None):
        """the whole write path in one call (what the bench times): src -> dense container + offsets.  For the shapes
        the fast encoder takes this is ONE launch (the container is built inside it, csrc/compact_tail.h); align 16 only."""
        if self.align != 16:
            raise ValueError("compress_dense builds the 16-byte aligned container; use compress_to_slots + compact for another alignment")
        nchunks = int(_lib.num_chunks(total_len, self.chunk_len))
        ws = ws or self.workspace(nchunks)
        dense, offsets = self._new_container(nchunks, dense, offsets)
        with self._on():
            _lib.check(_lib.compress_batch_dense(_CODEC_ID[self.codec], self.esz, src_padded_u8.data_ptr(), total_len,
                                                 self.chunk_len, self.ndims, ws["slots"].data_ptr(), self.slot_stride,
                                                 ws["sizes"].data_ptr(), ws["rets"].data_ptr(), dense.data_ptr(),
                                                 offsets.data_ptr(), ws["tmp"].data_ptr(), self._stream()))
        return ws, dense, offsets

    def compress(self, src):
        """src: device tensor of dtype uint8/uint16, any shape, row-major [.., ndims]."""
        t = self.torch
        if src.dtype.itemsize != self.esz or src.dtype.is_floating_point or src.device != self.device:
            raise ValueError(f"src must be a {self.esz}-byte integer tensor on {self.device}")
        total_len = src.numel()
        nchunks = int(_lib.num_chunks(total_len, self.chunk_len))
        if self.align == 16:
            ws, dense, offsets = self.compress_dense(self._padded_view(src.contiguous()), total_len)
        else:
            ws = self.compress_to_slots(self._padded_view(src.contiguous()), total_len)
            dense, offsets = self.compact(ws, nchunks)
        total = int(offsets[-1].item())
        data = dense[: total + _lib.READ_SLACK].clone()
        return CompressedBatch(data, offsets, ws["sizes"].clone(), nchunks, total_len, self.chunk_len, self.ndims)

    def compress_floats(self, src, scale=None, offset=None, signed=False, rounding="nearest"):
        """compress() of a float tensor that the encoder quantises while it loads: float_rows' way in, in one launch for the shapes
        compress() takes in one -- the integer tensor never exists.  Element x of column d is coded as
            q = clamp(round((x.float() - offset[d]) * (1 / scale[d])), LO, HI),   NaN -> 0,
        LO / HI the range of the codec's unsigned element type, or of the signed one with signed=True; the batch is byte for byte
        compress(q).  (scale, offset) are what float_rows takes -- a number, a sequence of ndims numbers or a tensor of ndims elements;
        None is all 1 / all 0 -- so compress_floats(x, *datasets.dequantize_params(m, dt)) and float_rows(batch, *dequantize_params(m, dt))
        are each other's way back; 1 / scale is one float32 division (rowops.quant_params).  rounding: "nearest" (ties to even) or
        "floor" -- which matches datasets.quantize's truncation within one step, not bit for bit: quantize divides in float32 where this
        multiplies by a reciprocal.

        src: a torch.float32, float16 or bfloat16 tensor on the codec's device, any shape, row-major [.., ndims]; a non-contiguous one
        is made contiguous (a copy).  chunk_len must be a multiple of ndims; the codec must be 'delta' or 'xff' with align 16.
        -> a CompressedBatch, as compress() returns it."""
        torch = self.torch
        if not torch.is_tensor(src):
            raise ValueError("src must be a float tensor")
        fmt = rowops.float_format(src.dtype)
        if src.device != self.device:
            raise ValueError(f"src must be on {self.device}")
        if self.align != 16:
            raise ValueError("compress_floats builds the 16-byte aligned container")
        if rounding not in ("nearest", "floor"):
            raise ValueError("rounding must be 'nearest' or 'floor'")
        D = self.ndims
        rowops.chunk_rows(self.chunk_len, D, "compress_floats")
        inv, off = rowops.quant_params(scale, offset, D, self.device)
        flat = src.contiguous().reshape(-1)
        total_len = flat.numel()
        nchunks = int(_lib.num_chunks(total_len, self.chunk_len))
        ws = self.workspace(nchunks)
        dense, offsets = self._new_container(nchunks)
        flags = (_lib.FLOAT_SIGNED if signed else 0) | (_lib.QUANT_FLOOR if rounding == "floor" else 0)
        if total_len == 0:                                  # (an empty tensor has no address to hand over)
            offsets.zero_()
            return CompressedBatch(dense[: _lib.READ_SLACK].clone(), offsets, ws["sizes"].clone(), 0, 0, self.chunk_len, D)
        with self._on():
            _lib.check(_lib.compress_batch_float_dense(_CODEC_ID[self.codec], self.esz, flat.data_ptr(), fmt,
                                                       inv.data_ptr() if inv is not None else None, off.data_ptr() if off is not None else None,
                                                       flags, total_len, self.chunk_len, D, ws["slots"].data_ptr(), self.slot_stride,
                                                       ws["sizes"].data_ptr(), ws["rets"].data_ptr(), dense.data_ptr(), offsets.data_ptr(),
                                                       ws["tmp"].data_ptr(), self._stream()))
        total = int(offsets[-1].item())
        data = dense[: total + _lib.READ_SLACK].clone()
        return CompressedBatch(data, offsets, ws["sizes"].clone(), nchunks, total_len, self.chunk_len, D)

    def decompress(self, batch, out=None, rets=None):
        """-> device tensor of total_len elements (chunk c at c*chunk_len)."""
        t = self.torch
        if out is None:
            out = t.empty(batch.nchunks * self.chunk_len, dtype=self.dtype, device=self.device)
        self.decompress_into(batch.data, batch.offsets, batch.nchunks, out, rets)
        return out[: batch.total_len]

    def decompress_into(self, data, offsets, nchunks, out, rets=None):
        """decode kernel only (what the bench times)"""
        with self._on():
            _lib.check(_lib.decompress_batch(_CODEC_ID[self.codec], self.esz, data.data_ptr(), offsets.data_ptr(), nchunks,
                                             self.chunk_len, self.ndims, out.data_ptr(),
                                             rets.data_ptr() if rets is not None else None, self._stream()))


    # ---- column-major matrices (BASELINE config 5): cols is a [ndims, col_stride] tensor, variable d in row d
    def compress_colmajor(self, cols, nrows=None):
        """cols[d, r] = sample r of variable d.  Chunk = chunk_len/ndims rows of all variables; the
        streams are what the reference produces for the row-major flattening of those rows."""
        if cols.dim() != 2 or cols.shape[0] != self.ndims or cols.dtype.itemsize != self.esz or not cols.is_contiguous():
            raise ValueError("cols must be a contiguous [ndims, col_stride] tensor of the codec's element type")
        if self.chunk_len % self.ndims:
            raise ValueError("chunk_len must be a multiple of ndims for column-major data")
        col_stride = int(cols.shape[1])
        nrows = col_stride if nrows is None else int(nrows)
        rows_per_chunk = self.chunk_len // self.ndims
        nchunks = (nrows + rows_per_chunk - 1) // rows_per_chunk
        ws = self.workspace(nchunks)
        if self.align == 16:                                # encode + container in one call (one launch where the encoder carries the tail)
            dense, offsets = self._new_container(nchunks)
            with self._on():
                _lib.check(_lib.compress_batch_colmajor_dense(_CODEC_ID[self.codec], self.esz, cols.data_ptr(), nrows, col_stride, rows_per_chunk,
                                                              self.ndims, ws["slots"].data_ptr(), self.slot_stride, ws["sizes"].data_ptr(),
                                                              ws["rets"].data_ptr(), dense.data_ptr(), offsets.data_ptr(), ws["tmp"].data_ptr(),
                                                              self._stream()))
        else:
            with self._on():
                _lib.check(_lib.compress_batch_colmajor(_CODEC_ID[self.codec], self.esz, cols.data_ptr(), nrows, col_stride, rows_per_chunk,
                                                        self.ndims, ws["slots"].data_ptr(), self.slot_stride, ws["sizes"].data_ptr(),
                                                        ws["rets"].data_ptr(), self._stream()))
            dense, offsets = self.compact(ws, nchunks)
        total = int(offsets[-1].item())
        return CompressedBatch(dense[: total + _lib.READ_SLACK].clone(), offsets, ws["sizes"].clone(), nchunks,
                               nrows * self.ndims, self.chunk_len, self.ndims)

    def decompress_colmajor(self, batch, out=None):
        """-> [ndims, nrows] tensor (out, if given: [ndims, col_stride >= nchunks*rows_per_chunk])"""
        t = self.torch
        rows_per_chunk = self.chunk_len // self.ndims
        nrows = batch.total_len // self.ndims
        if out is None:
            out = t.empty((self.ndims, batch.nchunks * rows_per_chunk), dtype=self.dtype, device=self.device)
        with self._on():
            _lib.check(_lib.decompress_batch_colmajor(_CODEC_ID[self.codec], self.esz, batch.data.data_ptr(), batch.offsets.data_ptr(),
                                                      batch.nchunks, rows_per_chunk, self.ndims, int(out.shape[1]), out.data_ptr(),
                                                      None, self._stream()))
        return out[:, :nrows]

    def query(self, batch, op, materialize=False, out=None, reduce=True):
        """Query on the compressed container (query.hpp:23-29): per-column max / sum fused into
        the decode; returns (result, out).  result: uint64 tensor [ndims] (reduce=True) or the
        per-chunk partials [nchunks, ndims]; out: the decompressed elements if materialize."""
        torch = self.torch
        n = batch.nchunks
        opid = {None: _lib.QUERY_NOOP, "noop": _lib.QUERY_NOOP, "max": _lib.QUERY_MAX, "sum": _lib.QUERY_SUM}[op]
        if materialize and out is None:
            out = torch.empty(n * self.chunk_len, dtype=self.dtype, device=self.device)
        partials = torch.empty((n, self.ndims), dtype=torch.int64, device=self.device) if opid else None
        with self._on():
            _lib.check(_lib.query_batch(_CODEC_ID[self.codec], self.esz, batch.data.data_ptr(), batch.offsets.data_ptr(), n,
                                        self.chunk_len, self.ndims, opid, int(bool(materialize)), 0,
                                        out.data_ptr() if materialize else None,
                                        partials.data_ptr() if opid else None, None, self._stream()))
        res = partials
        if opid and reduce:
            res = torch.empty(self.ndims, dtype=torch.int64, device=self.device)
            with self._on():
                _lib.check(_lib.query_reduce(opid, partials.data_ptr(), n, self.ndims, res.data_ptr(), self._stream()))
        return res, (out[: batch.total_len] if materialize else None)

    def _general(self, general_layout):
        return _lib.QUERY_GENERAL_LAYOUT if general_layout else 0

    def _rets(self, n, check):
        return self.torch.empty(n, dtype=self.torch.int64, device=self.device) if check else None

    def query_windows(self, batch, window_rows, ops=("min", "max", "sum"), general_layout=False, per_chunk=False, check=True):
        """Per-window min / max / sum of every column, fused into the decode (nothing but the results leaves the chip).

        per_chunk=True: the kernel's chunk-relative windows as they are, {op: [nchunks, nwin, ndims]} with
        nwin = ceil(ceil(chunk_len / ndims) / window_rows); window_rows a multiple of 8.
        Default: windows over the batch's rows -- window w covers rows [w*W, min((w+1)*W, rows)), rows =
        ceil(total_len / ndims) -- as {op: [nwindows, ndims]}.  That needs chunk_len % ndims == 0 and R = chunk_len / ndims
        either a multiple of W or a divisor of it (then the kernel takes one window a chunk and W / R chunks fold here; W == R counts as
        a divisor, as in aggregate_rows and moments_rows, so it is served whether or not R is a multiple of 8 -- rowops.plan_windows).
        window_rows below 1 is a ValueError in either mode.
        ops: any of "min", "max" (codec dtype), "sum" (int64) and, global windows only, "count" (int64) and "mean" (float64).
        Empty windows hold the identities (min all ones, max 0, sum 0).  check=True raises SprintzError naming the first
        damaged chunk."""
        torch = self.torch
        ops = rowops.normalise_ops(ops, ("min", "max", "sum", "count", "mean"), "min / max / sum / count / mean")
        if per_chunk and set(ops) & {"count", "mean"}:
            raise ValueError("count and mean exist for global windows only (per_chunk=False)")
        W, D, n = int(window_rows), self.ndims, batch.nchunks
        if not per_chunk and self.chunk_len % D:
            raise ValueError(f"global windows need chunk_len % ndims == 0 ({self.chunk_len} % {D}): use per_chunk=True")
        R, _ = rowops.chunk_rows(self.chunk_len, D)
        kw, fold, nwin = rowops.plan_windows(R, W, per_chunk)
        bits = (_lib.QUERY_WIN_MIN if "min" in ops else 0) | (_lib.QUERY_WIN_MAX if "max" in ops else 0) | \
               (_lib.QUERY_WIN_SUM if set(ops) & {"sum", "mean"} else 0)
        if bits == 0:                                       # count alone: no decode needed
            bits = _lib.QUERY_WIN_SUM
        shape = (n, nwin, D)
        res = {}
        if bits & _lib.QUERY_WIN_MIN:
            res["min"] = torch.empty(shape, dtype=self.dtype, device=self.device)
        if bits & _lib.QUERY_WIN_MAX:
            res["max"] = torch.empty(shape, dtype=self.dtype, device=self.device)
        if bits & _lib.QUERY_WIN_SUM:
            res["sum"] = torch.empty(shape, dtype=torch.int64, device=self.device)
        rets = self._rets(n, check)
        with self._on():
            _lib.check(_lib.query_windows(_CODEC_ID[self.codec], self.esz, batch.data.data_ptr(), batch.offsets.data_ptr(), n,
                                          self.chunk_len, D, kw, bits, self._general(general_layout),
                                          res["min"].data_ptr() if "min" in res else None,
                                          res["max"].data_ptr() if "max" in res else None,
                                          res["sum"].data_ptr() if "sum" in res else None,
                                          rets.data_ptr() if rets is not None else None, self._stream()))
        if check:
            rowops.raise_damaged("query_windows", rets, n, _lib.SprintzError)
        if per_chunk:
            return {k: v for k, v in res.items() if k in ops}
        out = rowops.fold_windows(res, n, nwin, D, W, fold, batch.total_len, self.esz, self.dtype)
        if set(ops) & {"count", "mean"}:
            # column d of window w: the full rows of the window, plus the partial last row where it reaches column d
            nw = -(-(-(-batch.total_len // D)) // W)
            full, part = divmod(batch.total_len, D)
            w0 = torch.arange(nw, dtype=torch.int64, device=self.device) * W
            cnt = (torch.clamp(torch.clamp(w0 + W, max=full) - w0, min=0))[:, None].expand(nw, D).clone()
            if part:
                wl = full // W
                cnt[wl, :part] += 1
            out["count"] = cnt
            if "mean" in ops:
                out["mean"] = out["sum"].to(torch.float64) / cnt.to(torch.float64)
        return {k: v for k, v in out.items() if k in ops}

    def gather_rows(self, batch, starts, rows, out=None, rets=None, check=True):
        """N row ranges of the compressed batch, decoded in one launch -> tensor [N, rows, ndims] of the codec's dtype.

        Batch row g is row g % R of chunk g / R, R = chunk_len / ndims (chunk_len must be a multiple of ndims); range i is
        batch rows [starts[i], starts[i] + rows).  starts: an int64 / uint64 device tensor, or anything torch.as_tensor
        takes.  Ranges may overlap, repeat and span chunks; a chunk several ranges touch is decoded once per range.
        check=True allocates `rets` if none was given and raises SprintzError naming the first range that needs a row the
        batch does not hold or touches a damaged chunk (damage behind the last row a range needs from a chunk may go
        unnoticed); check=False does not synchronise -- pass `rets` [N] int64 to look at the outcome later."""
        torch = self.torch
        if not torch.is_tensor(starts) or starts.dtype not in (torch.int64, torch.uint64) or starts.device != self.device:
            starts = torch.as_tensor(starts, dtype=torch.int64).to(self.device)
        starts = starts.reshape(-1).contiguous()
        n, rows, D = int(starts.numel()), int(rows), self.ndims
        if rows < 1:
            raise ValueError("rows must be positive")
        if out is None:
            out = torch.empty((n, rows, D), dtype=self.dtype, device=self.device)
        elif out.dtype != self.dtype or out.device != self.device or out.numel() != n * rows * D or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous {self.dtype} tensor of {n} x {rows} x {D} elements on {self.device}")
        if rets is None and check:
            rets = torch.empty(n, dtype=torch.int64, device=self.device)
        if rets is not None and (rets.dtype != torch.int64 or rets.device != self.device or rets.numel() < n or not rets.is_contiguous()):
            raise ValueError(f"rets must be a contiguous int64 tensor of at least {n} entries on {self.device}")
        if n == 0:
            return out.view(0, rows, D)
        with self._on():
            _lib.check(_lib.gather_rows(_CODEC_ID[self.codec], self.esz, batch.data.data_ptr(), batch.offsets.data_ptr(), batch.nchunks,
                                        self.chunk_len, D, starts.data_ptr(), n, rows, out.data_ptr(),
                                        rets.data_ptr() if rets is not None else None, self._stream()))
        i = rowops.first_bad(rets, n) if check else None
        if i is not None:
            code = int(rets[i].item())
            what = "needs a row the batch does not hold" if code == _lib.E_INVALID else "touches a damaged chunk"
            raise _lib.SprintzError(code, f"gather_rows: range {i} (start {int(starts[i].item())}) {what} (decoder returned {code})")
        return out.view(n, rows, D)

    def _filter_bounds(self, lo, hi, mode):
        """lo / hi: a scalar, a sequence of ndims entries (None = open end) or a device tensor -> two contiguous device tensors [ndims]"""
        return rowops.filter_bounds(lo, hi, mode, self.ndims, self.esz, self.dtype, self.device)

    def zone_map(self, batch, general_layout=False):
        """The batch's zone map: every chunk's per-column minimum and maximum and its element count, in one launch (query_windows with one
        window a chunk) -> ZoneMap.  Build it once and pass it as zones= to filter_rows, filter_linear and the *_where operations: the
        chunks whose bounds already decide the predicate are then not decoded.  The map holds for the container as it is now, for this
        general_layout and for the SPRINTZ_OPT_REF_DECODER_QUIRK state of the moment; a damaged chunk is recorded (len < 0), not raised."""
        torch = self.torch
        n, D = batch.nchunks, self.ndims
        zmin = torch.empty((n, D), dtype=self.dtype, device=self.device)
        zmax = torch.empty((n, D), dtype=self.dtype, device=self.device)
        zlen = torch.empty(n, dtype=torch.int64, device=self.device)
        with self._on():
            _lib.check(_lib.zone_map(_CODEC_ID[self.codec], self.esz, batch.data.data_ptr(), batch.offsets.data_ptr(), n, self.chunk_len, D,
                                     self._general(general_layout), zmin.data_ptr(), zmax.data_ptr(), zlen.data_ptr(), self._stream()))
        return ZoneMap(zmin, zmax, zlen, bool(general_layout), _lib.ref_decoder_quirk())

    def _filter_launch(self, op, batch, MB, zones, general_layout, check, prune, launch):
        """A filter's outputs {"mask", "counts"} in batch order, pruned by `zones` where they are given.  launch(offsets_ptr, n, mask, counts,
        rets) is the filter's entry point on a container of n chunks; prune(cls, pos, surv, tmp) the prune call of its predicate, or None
        where the predicate cannot be pruned: the zones are then checked and not used.  self.last_prune is what THIS call pruned.  With zones:
        prune, read the survivor count n' (8 bytes: the call's one synchronisation), then the plain call if every chunk survived, else the
        filter on the survivors' offsets into compact buffers (nothing if n' == 0) and the expand launch."""
        torch = self.torch
        n = batch.nchunks
        mask = torch.empty((n, MB), dtype=torch.uint8, device=self.device)
        counts = torch.empty(n, dtype=torch.int32, device=self.device)
        rets = self._rets(n, check)
        self.last_prune = None
        if zones is not None:
            rowops.check_zones(zones, n, self.ndims, general_layout, _lib.ref_decoder_quirk())
        with self._on():
            ns = n
            if zones is not None and prune is not None and n:
                cls = torch.empty(n, dtype=torch.uint8, device=self.device)
                pos = torch.empty(n + 1, dtype=torch.int64, device=self.device)
                surv = torch.empty(n + 1, dtype=torch.int64, device=self.device)
                tmp = torch.empty(_lib.zone_prune_tmp_bytes(n) // 8, dtype=torch.int64, device=self.device)
                _lib.check(prune(cls, pos, surv, tmp))
                ns = int(pos[n].item())
                self.last_prune = {"nchunks": n, "survivors": ns, "class": cls}
            if ns == n:
                _lib.check(launch(batch.offsets.data_ptr(), n, mask, counts, rets))
            else:
                cmask = ccounts = crets = None
                if ns:
                    cmask = torch.empty((ns, MB), dtype=torch.uint8, device=self.device)
                    ccounts = torch.empty(ns, dtype=torch.int32, device=self.device)
                    crets = self._rets(ns, check)
                    _lib.check(launch(surv.data_ptr(), ns, cmask, ccounts, crets))
                _lib.check(_lib.zone_expand(n, self.chunk_len, self.ndims, cls.data_ptr(), pos.data_ptr(), zones.len.data_ptr(), _ptr(cmask),
                                            _ptr(ccounts), _ptr(crets), mask.data_ptr(), counts.data_ptr(), _ptr(rets), self._stream()))
        if check:
            rowops.raise_damaged(op, rets, n, _lib.SprintzError)
        return {"mask": mask, "counts": counts}

    def filter_rows(self, batch, lo, hi, mode="all", general_layout=False, ids=False, check=True, zones=None):
        """Which rows satisfy a condition on their columns, straight from the compressed batch (one launch, no sample leaves the chip).

        A row matches under mode="all" if every column d has lo[d] <= x <= hi[d] (unsigned, inclusive), under mode="any" if some
        column has.  lo / hi: a scalar, a sequence of ndims entries, or a device tensor of the codec's dtype; a None entry is an
        open end (0 / the type's maximum), and a column with neither bound is unconstrained: it always matches under "all" and
        never -- an empty interval -- under "any".
        -> {"mask": uint8 [nchunks, MB], "counts": int32 [nchunks]}: bit r & 7 of mask[c, r >> 3] is row r of chunk c, MB =
        ceil(ceil(chunk_len / ndims) / 8); rows that do not exist (a short last chunk, a partial last row) are 0.
        ids=True adds "ids": int64 [total], the matching batch rows in ascending order (row g is row g % R of chunk g // R, R =
        chunk_len / ndims: chunk_len must be a multiple of ndims) -- what gather_rows takes as starts.
        check=True raises SprintzError naming the first damaged chunk.  ids=True checks too, whatever check says: a damaged chunk's
        count is unspecified, and it would size the ids and place every later chunk's.
        zones: the batch's ZoneMap (zone_map).  The results are the same bit for bit; the chunks whose minimum and maximum already decide
        the predicate -- no row can match, or every row does -- are not decoded: a prune launch classifies the chunks, the filter runs on
        the survivors alone and an expand launch puts its results back in batch order.  That costs one 8-byte read of the survivor
        count, the call's single synchronisation (check=False does not avoid it).  A damaged chunk is named by its batch number, as
        without zones.  A map built under another general_layout or SPRINTZ_OPT_REF_DECODER_QUIRK state is a ValueError.
        self.last_prune then holds {"nchunks": n, "survivors": n', "class": uint8 [n] of 0 NONE / 1 ALL / 2 DECODE}; after a filter call that
        pruned nothing -- no zones, an empty batch, filter_linear with a lag term -- it is None."""
        check = check or ids
        if mode not in ("all", "any"):
            raise ValueError("mode must be 'all' or 'any'")
        D = self.ndims
        R, MB = rowops.chunk_rows(self.chunk_len, D, "ids" if ids else None, verb="need")
        lo_t, hi_t = self._filter_bounds(lo, hi, mode)
        cid, flags, fmode, st = _CODEC_ID[self.codec], self._general(general_layout), _lib.FILTER_ALL if mode == "all" else _lib.FILTER_ANY, self._stream()

        def launch(offsets, n, mask, counts, rets):
            return _lib.filter_rows(cid, self.esz, batch.data.data_ptr(), offsets, n, self.chunk_len, D, lo_t.data_ptr(), hi_t.data_ptr(), fmode,
                                    flags, mask.data_ptr(), counts.data_ptr(), _ptr(rets), st)

        def prune(cls, pos, surv, tmp):
            return _lib.zone_prune_box(self.esz, batch.nchunks, self.chunk_len, D, batch.offsets.data_ptr(), zones.min.data_ptr(),
                                       zones.max.data_ptr(), zones.len.data_ptr(), lo_t.data_ptr(), hi_t.data_ptr(), fmode, cls.data_ptr(),
                                       pos.data_ptr(), surv.data_ptr(), tmp.data_ptr(), st)

        res = self._filter_launch("filter_rows", batch, MB, zones, general_layout, check, prune, launch)
        if ids:
            res["ids"] = self._mask_ids(res["mask"], res["counts"])
        return res

    def _mask_ids(self, mask, counts):
        """a filter's mask and counts -> int64 [total]: the matching batch rows in ascending order (a prefix sum of the counts and the
        filter_row_ids launch)"""
        torch = self.torch
        n = counts.numel()
        incl = torch.cumsum(counts.to(torch.int64), 0)
        total = int(incl[-1].item()) if n else 0
        out = torch.empty(total, dtype=torch.int64, device=self.device)
        if total:
            bases = (incl - counts).contiguous()
            with self._on():
                _lib.check(_lib.filter_row_ids(mask.data_ptr(), bases.data_ptr(), n, self.chunk_len, self.ndims, out.data_ptr(), total, self._stream()))
        return out

    def filter_linear(self, batch, weights, lo=None, hi=None, lag_weights=None, bias=0, general_layout=False, ids=False, check=True, zones=None):
        """Which rows satisfy a condition that RELATES columns, or a row to the row in front of it -- filter_rows' second kind of
        predicate, straight from the compressed batch.  Batch row g (row g % R of chunk g // R, R = chunk_len / ndims: chunk_len must be
        a multiple of ndims) matches if

            lo <= bias + sum_d weights[d] x[g, d] + sum_d lag_weights[d] x[g - 1, d] <= hi

        with x the unsigned samples as integers; row 0 is its own predecessor (numpy.diff(..., prepend=x[0])).  weights / lag_weights:
        a scalar (every column), a sequence of ndims entries, a dict {column: weight} or an integer tensor; lag_weights=None: no lag
        term.  lo / hi: signed, inclusive, None = open.  The sum is exact: a form that could pass 2^31 in magnitude is a ValueError
        (rowops.linear_terms).
        -> filter_rows' dict, in its layout: {"mask": uint8 [nchunks, MB], "counts": int32 [nchunks]} and, with ids=True, "ids".  The masks
        of both filters combine with & / | in torch and feed select_rows, aggregate_rows and the other mask consumers unchanged:

            m = codec.filter_linear(batch, {0: 1, 1: -1}, lo=1)["mask"]                  # WHERE a > b
            rows = codec.select_rows(batch, m & codec.filter_rows(batch, lo, hi)["mask"])["rows"]

        check=True raises SprintzError naming the first damaged chunk; ids=True checks too (as filter_rows).
        zones: the batch's ZoneMap, as in filter_rows -- the form's range over a chunk follows from the chunk's minima and maxima, and a chunk
        whose range lies outside [lo, hi], or inside it, is not decoded; the results are the same bit for bit.  With lag_weights the
        zones are checked as always (a map of another batch, layout or quirk state is a ValueError) and then ignored, and the call runs unpruned: the seam pass takes each chunk's predecessor from its neighbour in launch order,
        and a launch on the survivors alone has other neighbours."""
        torch = self.torch
        check = check or ids
        D, n = self.ndims, batch.nchunks
        R, MB = rowops.chunk_rows(self.chunk_len, D, "filter_linear")
        w, u, bias, lo, hi = rowops.linear_terms(weights, lag_weights, bias, lo, hi, D, self.esz, self.device)
        tmp = torch.empty(max(_lib.filter_linear_tmp_bytes(self.esz, n, D) // 8, 1), dtype=torch.int64, device=self.device) if u is not None else None
        cid, flags, st = _CODEC_ID[self.codec], self._general(general_layout), self._stream()

        def launch(offsets, n, mask, counts, rets):
            return _lib.filter_linear(cid, self.esz, batch.data.data_ptr(), offsets, n, self.chunk_len, D, w.data_ptr(), _ptr(u), bias, lo, hi,
                                      flags, _ptr(tmp), mask.data_ptr(), counts.data_ptr(), _ptr(rets), st)

        def prune(cls, pos, surv, ztmp):                    # (no lag term)
            return _lib.zone_prune_linear(self.esz, batch.nchunks, self.chunk_len, D, batch.offsets.data_ptr(), zones.min.data_ptr(),
                                          zones.max.data_ptr(), zones.len.data_ptr(), w.data_ptr(), bias, lo, hi, cls.data_ptr(),
                                          pos.data_ptr(), surv.data_ptr(), ztmp.data_ptr(), st)

        res = self._filter_launch("filter_linear", batch, MB, zones, general_layout, check, prune if u is None else None, launch)
        if ids:
            res["ids"] = self._mask_ids(res["mask"], res["counts"])
        return res

    def filter_change(self, batch, col, lo=None, hi=None, **kw):
        """Which rows CHANGE: lo <= x[g, col] - x[g - 1, col] <= hi (filter_linear with weights e_col and lag_weights -e_col; row 0
        changes by 0).  Spikes and steps are two calls, the change log of a state column one:

            up, down = codec.filter_change(batch, 3, lo=t + 1)["mask"], codec.filter_change(batch, 3, hi=-t - 1)["mask"]   # |dx| > t: up | down
            log = codec.filter_change(batch, 0, lo=0, hi=0)      # state[r] == state[r-1]: ~mask over the rows that exist is the event log
            events = codec.filter_change(batch, 0, lo=1, ids=True)["ids"]      # ... or the rows where the state went up, by number"""
        return self.filter_linear(batch, {int(col): 1}, lo=lo, hi=hi, lag_weights={int(col): -1}, **kw)

    def _where(self, op, method, batch, lo, hi, mode, /, counts=False, zones=None, **kw):
        """filter_rows (lo / hi / mode), then `method` on its mask (counts=True: and its counts).  Whole rows are asked for before the
        filter launches.  zones: the batch's ZoneMap for the filter step -- that half alone is pruned, `method` decodes every chunk."""
        rowops.chunk_rows(self.chunk_len, self.ndims, op)
        f = self.filter_rows(batch, lo, hi, mode=mode, general_layout=kw.get("general_layout", False), check=True, zones=zones)
        if counts:
            kw["counts"] = f["counts"]
        return method(batch, mask=f["mask"], **kw)

    def select_rows(self, batch, mask, counts=None, out=None, ids=False, general_layout=False, check=True):
        """The rows a mask names, packed densely: every chunk decoded once, only the selected rows stored (one launch).

        mask: uint8 [nchunks, MB] in filter_rows' layout (bit r & 7 of mask[c, r >> 3] is row r of chunk c, MB = ceil(R / 8),
        R = chunk_len / ndims: chunk_len must be a multiple of ndims) -- from filter_rows, several of its masks combined, or anywhere
        else; bits of rows that do not exist are ignored.  counts: the set bits of every chunk over the rows that exist (int32 / int64
        [nchunks], as filter_rows returns them); without them a device popcount of the mask over rows 0 .. R-1 stands in, which is
        right for masks that are 0 where no row exists (filter_rows' are).
        -> {"rows": [total, ndims] of the codec's dtype}, plus "ids": int64 [total] -- the rows' batch row numbers -- with ids=True;
        ascending batch row order.  out: a contiguous tensor of at least total * ndims elements to write into.
        check=True raises SprintzError naming the first damaged chunk."""
        torch = self.torch
        D, n = self.ndims, batch.nchunks
        R, MB = rowops.chunk_rows(self.chunk_len, D, "select_rows")
        mask = rowops.check_mask(mask, n, MB, self.device)
        if counts is None:
            m = mask.view(n, MB).to(torch.int32)
            if R % 8:
                m[:, -1] &= (1 << (R % 8)) - 1
            counts = sum(((m >> b) & 1).sum(dim=1) for b in range(8)) if n else m.new_zeros(0)
        elif not torch.is_tensor(counts) or counts.device != self.device or counts.numel() != n:
            raise ValueError(f"counts must be a tensor of {n} entries on {self.device}")
        counts = counts.reshape(-1).to(torch.int64)
        incl = torch.cumsum(counts, 0)
        total = int(incl[-1].item()) if n else 0
        if out is None:
            out = torch.empty(total * D, dtype=self.dtype, device=self.device)
        elif out.dtype != self.dtype or out.device != self.device or out.numel() < total * D or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous {self.dtype} tensor of at least {total} x {D} elements on {self.device}")
        res = {"rows": out.view(-1)[: total * D].view(total, D)}
        if ids:
            res["ids"] = torch.empty(total, dtype=torch.int64, device=self.device)
        if n == 0:
            return res
        bases = (incl - counts).contiguous()
        rets = self._rets(n, check)
        dest = out if out.numel() else torch.empty(D, dtype=self.dtype, device=self.device)   # (no row selected: the chunks are still checked)
        with self._on():
            _lib.check(_lib.select_rows(_CODEC_ID[self.codec], self.esz, batch.data.data_ptr(), batch.offsets.data_ptr(), n,
                                        self.chunk_len, D, mask.data_ptr(), bases.data_ptr(), total, self._general(general_layout),
                                        dest.data_ptr(), res["ids"].data_ptr() if ids else None,
                                        rets.data_ptr() if rets is not None else None, self._stream()))
        if check:
            rowops.raise_damaged("select_rows", rets, n, _lib.SprintzError)
        return res

    def float_rows(self, batch, dtype=None, scale=None, offset=None, signed=False, out=None, rets=None, general_layout=False, check=True):
        """The batch decoded straight into floats: element x of column d leaves as (x.to(float32) * scale[d] + offset[d]).to(dtype), bit
        for bit what torch computes on the CPU, in one launch -- the integer tensor never exists.

        dtype: torch.float32 (the default), torch.float16 or torch.bfloat16.  scale / offset: a number, a sequence of ndims numbers or
        a tensor of ndims elements (host values must be finite); None is all 1 / all 0.  signed=True reads the elements as int8 / int16.
        chunk_len must be a multiple of ndims.  datasets.dequantize_params gives the scale and offset that invert datasets.quantize.
        -> a tensor of batch.total_len elements of dtype (chunk c at c * chunk_len), viewed [rows, ndims] when total_len % ndims == 0.
        out: a contiguous tensor of dtype with at least nchunks * chunk_len elements to write into; rets: an int64 tensor of nchunks
        entries for the per-chunk element counts.  check=True raises SprintzError naming the first damaged chunk."""
        torch = self.torch
        dtype = torch.float32 if dtype is None else dtype
        fmt = rowops.float_format(dtype)
        D, n = self.ndims, batch.nchunks
        rowops.chunk_rows(self.chunk_len, D, "float_rows")
        scale = rowops.float_params(scale, D, "scale", self.device)
        offset = rowops.float_params(offset, D, "offset", self.device)
        if out is None:
            out = torch.empty(n * self.chunk_len, dtype=dtype, device=self.device)
        elif not torch.is_tensor(out) or out.dtype != dtype or out.device != self.device or out.numel() < n * self.chunk_len or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous {dtype} tensor of at least {n} x {self.chunk_len} elements on {self.device}")
        if rets is None:
            rets = self._rets(n, check)
        if n:
            with self._on():
                _lib.check(_lib.float_rows(_CODEC_ID[self.codec], self.esz, batch.data.data_ptr(), batch.offsets.data_ptr(), n,
                                           self.chunk_len, D, fmt, scale.data_ptr() if scale is not None else None,
                                           offset.data_ptr() if offset is not None else None,
                                           self._general(general_layout) | (_lib.FLOAT_SIGNED if signed else 0), out.data_ptr(),
                                           rets.data_ptr() if rets is not None else None, self._stream()))
            if check:
                rowops.raise_damaged("float_rows", rets, n, _lib.SprintzError)
        res = out.view(-1)[: batch.total_len]
        return res.view(-1, D) if batch.total_len % D == 0 else res

    def rolling_rows(self, batch, window_rows, ops=("min", "max", "sum"), general_layout=False, check=True):
        """Sliding-window min / max / sum / mean of every column, one result per row -- pandas' rolling(window_rows, min_periods=1) --
        straight from the compressed batch: the decoded tensor never exists.  Batch row g is row g % R of chunk g // R, R = chunk_len /
        ndims (chunk_len must be a multiple of ndims), and out[g, d] = op(x[max(0, g - W + 1) .. g, d]): a trailing window, clipped at the
        batch's first row.

        window_rows: W, a multiple of 8 with 8 <= W <= R (rowops.rolling_window); the library refuses a window whose history does not fit
        the kernel's LDS and names the largest it takes.  ops: any of "min", "max" (the codec's dtype), "sum" (int32) and "mean" (float32:
        the sum launch plus one divide by the row's count min(g + 1, W)).
        -> {op: [G, ndims]}, G = ceil(total_len / ndims); the columns a partial last row lacks hold 0.  One library call: the decode and,
        with more than one chunk, its seam pass.  check=True raises SprintzError naming the first damaged chunk."""
        torch = self.torch
        ops = rowops.normalise_ops(ops, rowops.ROLLING_OPS, '"min", "max", "sum", "mean"')
        D, n = self.ndims, batch.nchunks
        R, _ = rowops.chunk_rows(self.chunk_len, D, "rolling_rows")
        W = rowops.rolling_window(window_rows, R, self.esz)
        G = -(-batch.total_len // D)
        want_sum = "sum" in ops or "mean" in ops
        bits = (_lib.ROLL_MIN if "min" in ops else 0) | (_lib.ROLL_MAX if "max" in ops else 0) | (_lib.ROLL_SUM if want_sum else 0)
        raw = {}
        for name, dt in (("min", self.dtype), ("max", self.dtype), ("sum", torch.int32)):
            if name in ops or (name == "sum" and want_sum):
                raw[name] = torch.empty(max(n * self.chunk_len, 1), dtype=dt, device=self.device)
        tmp = torch.empty(max(rowops.rolling_tmp_bytes(n, W, D, self.esz) // 16, 1) * 2, dtype=torch.int64, device=self.device)
        rets = self._rets(n, check)
        if n:
            with self._on():
                _lib.check(_lib.rolling_rows(_CODEC_ID[self.codec], self.esz, batch.data.data_ptr(), batch.offsets.data_ptr(), n, self.chunk_len, D,
                                             W, bits, self._general(general_layout), _ptr(raw.get("min")), _ptr(raw.get("max")), _ptr(raw.get("sum")),
                                             tmp.data_ptr(), _ptr(rets), self._stream()))
            if check:
                rowops.raise_damaged("rolling_rows", rets, n, _lib.SprintzError)
        res = {}
        for name, v in raw.items():
            v = v[: G * D]
            v[batch.total_len:] = 0
            res[name] = v.view(G, D)
        if "mean" in ops:
            res["mean"] = rowops.rolling_mean(res["sum"], rowops.rolling_counts(G, W, self.device))
            if "sum" not in ops:
                del res["sum"]
        return {k: res[k] for k in ops}

    def project_rows(self, batch, columns, dtype=None, scale=None, offset=None, signed=False, out=None, rets=None, general_layout=False, check=True):
        """SELECT a, b: the columns `columns` names, decoded straight into a dense [G, K] tensor, G = ceil(total_len / ndims) -- out[g, j] =
        x[g, columns[j]] -- in one launch; the other columns are never stored, and the full tensor never exists.

        columns: K >= 1 distinct column numbers in 0 .. ndims - 1, in any order (rowops.project_slots).  dtype: None for the codec's dtype,
        or torch.float32 / torch.float16 / torch.bfloat16 for float_rows' conversion, (x.to(float32) * scale[j] + offset[j]).to(dtype), bit
        for bit what torch computes on the CPU.  scale / offset: float_rows' forms with K entries, indexed by output column, a float dtype
        only; signed=True reads the elements as int8 / int16, a float dtype only.  chunk_len must be a multiple of ndims.
        -> a [G, K] tensor; where the batch ends mid-row, the columns that last row lacks hold 0.  out: a contiguous tensor of the output
        dtype with at least nchunks x R x K elements (a chunk slot each chunk, R = chunk_len / ndims) to write into -- its first G x K are the result; rets: an int64 tensor of nchunks entries for the per-chunk element counts (of
        all ndims columns, as decompress reports them).  check=True raises SprintzError naming the first damaged chunk."""
        torch = self.torch
        D, n = self.ndims, batch.nchunks
        R, _ = rowops.chunk_rows(self.chunk_len, D, "project_rows")
        slots = rowops.project_slots(columns, D, self.device)
        K = int((slots >= 0).sum())
        if dtype is None or dtype == self.dtype:
            if scale is not None or offset is not None or signed:
                raise ValueError("scale, offset and signed go with a float dtype")
            dtype, fmt = self.dtype, _lib.PROJECT_RAW
        else:
            fmt = 1 + rowops.float_format(dtype)
            scale = rowops.float_params(scale, K, "scale", self.device)
            offset = rowops.float_params(offset, K, "offset", self.device)
        G = -(-batch.total_len // D)
        if out is None:
            out = torch.empty(n * R * K, dtype=dtype, device=self.device)
        elif not torch.is_tensor(out) or out.dtype != dtype or out.device != self.device or out.numel() < n * R * K or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous {dtype} tensor of at least {n} x {R} x {K} elements on {self.device}")
        if rets is None:
            rets = self._rets(n, check)
        res = out.view(-1)[: G * K].view(G, K)
        if n:
            with self._on():
                _lib.check(_lib.project_rows(_CODEC_ID[self.codec], self.esz, batch.data.data_ptr(), batch.offsets.data_ptr(), n, self.chunk_len, D,
                                             slots.data_ptr(), K, fmt, _ptr(scale), _ptr(offset),
                                             self._general(general_layout) | (_lib.FLOAT_SIGNED if signed else 0), out.data_ptr(), _ptr(rets), self._stream()))
            if check:
                rowops.raise_damaged("project_rows", rets, n, _lib.SprintzError)
            if batch.total_len % D:                        # the batch ends mid-row: the columns that row lacks are not written
                there = slots[: batch.total_len % D]
                lacks = torch.ones(K, dtype=torch.bool, device=self.device)
                lacks[there[there >= 0].long()] = False
                # (zero bits through a signed view of the same width: torch fills no uint16 tensor under a mask)
                res.view({1: torch.int8, 2: torch.int16, 4: torch.int32}[res.element_size()])[G - 1, lacks] = 0
        return res

    def derive_rows(self, batch, forms, lag_forms=None, bias=0, dtype=None, scale=None, offset=None, prev=None, out=None, rets=None,
                    general_layout=False, check=True):
        """SELECT <expression>: K linear forms of every row, and of the row in front of it, decoded straight into a dense [G, K] tensor, G =
        total_len // ndims -- filter_linear's sum itself, returned instead of tested; the integer tensor never exists.  For batch row g (row
        g % R of chunk g // R, R = chunk_len / ndims: chunk_len must be a multiple of ndims; only whole rows are rows) and form k

            out[g, k] = bias[k] + sum_d forms[k][d] x[g, d] + sum_d lag_forms[k][d] x[g - 1, d]

        with x the unsigned samples as integers; row 0 is its own predecessor (numpy.diff(..., prepend=x[0])) unless prev gives the row in
        front of it -- ndims entries, the last row of the batch before this one: a stream continued over batches then differentiates exactly.
        forms / lag_forms: an integer tensor [K, ndims] or a sequence of K entries, each as filter_linear takes its weights (a scalar, a
        sequence of ndims entries, a dict {column: weight}, a tensor); 1 <= K <= 16; lag_forms=None: no lag term (and prev is ignored).  bias: a
        scalar or K entries.  Every form is exact: one that could reach 2^31 in magnitude is a ValueError (rowops.derive_forms).

            spread = codec.derive_rows(batch, [{0: 1, 1: -1}])                               # SELECT a - b            -> int32 [G, 1]
            both = codec.derive_rows(batch, [{0: 1, 1: -1}, {2: 1, 3: 1, 4: 1}])             # SELECT a - b, c + d + e -> int32 [G, 2]
            volts = codec.derive_rows(batch, [{0: 1, 1: -1}], dtype=torch.float32, scale=0.01)
            step = codec.derive_rows(batch, [{3: 1}], lag_forms=[{3: -1}])                   # x[g, 3] - x[g - 1, 3]: diff() of one column

        dtype: None or torch.int32 for the sums themselves, or torch.float32 / torch.float16 / torch.bfloat16 for
        (s.to(float32) * scale[k] + offset[k]).to(dtype), bit for bit what torch computes on the CPU; scale / offset: float_rows' forms with K
        entries, a float dtype only.
        -> a [G, K] tensor.  out: a contiguous tensor of the output dtype with at least nchunks x R x K elements (a chunk slot each chunk) to
        write into -- its first G x K are the result; rets: an int64 tensor of nchunks entries for the per-chunk element counts (as decompress
        reports them).  One library call: the decode and, with a lag term, its seam pass.  A damaged chunk's rows are unspecified, and row 0 of
        the chunk behind it; check=True raises SprintzError naming the first damaged chunk."""
        torch = self.torch
        D, n = self.ndims, batch.nchunks
        R, _ = rowops.chunk_rows(self.chunk_len, D, "derive_rows")
        w, u, b = rowops.derive_forms(forms, lag_forms, bias, D, self.esz, self.device)
        K = int(w.shape[0])
        if dtype is None or dtype == torch.int32:
            if scale is not None or offset is not None:
                raise ValueError("scale and offset go with a float dtype")
            dtype, fmt = torch.int32, _lib.DERIVE_I32
        else:
            fmt = 1 + rowops.float_format(dtype)
            scale = rowops.float_params(scale, K, "scale", self.device)
            offset = rowops.float_params(offset, K, "offset", self.device)
        if prev is not None and u is not None:
            prev = rowops.elem_tensor(prev, D, self.esz, self.dtype, self.device, "prev")
        else:
            prev = None
        G = batch.total_len // D
        if out is None:
            out = torch.empty(n * R * K, dtype=dtype, device=self.device)
        elif not torch.is_tensor(out) or out.dtype != dtype or out.device != self.device or out.numel() < n * R * K or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous {dtype} tensor of at least {n} x {R} x {K} elements on {self.device}")
        if rets is None:
            rets = self._rets(n, check)
        tmp = torch.empty(max(_lib.derive_rows_tmp_bytes(self.esz, n, D) // 8, 1), dtype=torch.int64, device=self.device) if u is not None else None
        res = out.view(-1)[: G * K].view(G, K)
        if n:
            with self._on():
                _lib.check(_lib.derive_rows(_CODEC_ID[self.codec], self.esz, batch.data.data_ptr(), batch.offsets.data_ptr(), n, self.chunk_len, D, K,
                                            w.data_ptr(), _ptr(u), b.data_ptr(), fmt, _ptr(scale), _ptr(offset), _ptr(prev),
                                            self._general(general_layout), _ptr(tmp), out.data_ptr(), _ptr(rets), self._stream()))
            if check:
                rowops.raise_damaged("derive_rows", rets, n, _lib.SprintzError)
        return res

    def diff_rows(self, batch, columns=None, **kw):
        """pandas' diff(): out[g, j] = x[g, columns[j]] - x[g - 1, columns[j]] as int32 (derive_rows with forms e_c and lag_forms -e_c; row 0
        changes by 0, or by its distance to prev's row where prev is given).  columns: up to 16 column numbers, None for all of them -- more
        than 16 is a ValueError: call it once per 16 columns.  Every other argument is derive_rows'.

            d = codec.diff_rows(batch)                         # torch.diff(x.to(int32), dim=0, prepend=x[:1])
            d = codec.diff_rows(batch, [3], dtype=torch.float32, scale=0.5)"""
        cols = list(range(self.ndims)) if columns is None else (columns.tolist() if self.torch.is_tensor(columns) or isinstance(columns, np.ndarray) else list(columns))
        if not cols:
            raise ValueError("columns must name at least one column")
        if len(cols) > rowops.DERIVE_MAX_FORMS:
            raise ValueError(f"diff_rows takes at most {rowops.DERIVE_MAX_FORMS} columns a call (derive_rows' forms), not {len(cols)}: call it once per {rowops.DERIVE_MAX_FORMS} columns")
        for c in cols:
            if isinstance(c, bool) or not isinstance(c, (int, np.integer)) or not 0 <= c < self.ndims:
                raise ValueError(f"column {c!r} is not an int in 0 .. {self.ndims - 1}")
        for name in ("forms", "lag_forms"):
            if name in kw:
                raise ValueError(f"diff_rows builds {name} itself")
        return self.derive_rows(batch, [{int(c): 1} for c in cols], lag_forms=[{int(c): -1} for c in cols], **kw)

    def fir_rows(self, batch, taps, bias=0, dtype=None, scale=None, offset=None, prev=None, return_tail=False, out=None, rets=None,
                 general_layout=False, check=True):
        """A per-column tap filter over the rows -- a weighted history of every column -- straight from the compressed batch; the decoded tensor
        never exists.  For batch row g (row g % R of chunk g // R, R = chunk_len / ndims: chunk_len must be a multiple of ndims) and column d

            out[g, d] = bias[d] + sum_{j = 0 .. T - 1} taps[j][d] x[g - j, d]

        with x the unsigned samples as integers; taps[0] weighs the row itself.  taps: T integers shared by all columns, or [T, ndims] (a
        sequence or an integer tensor); 1 <= T <= 256 and T - 1 <= R.  bias: a scalar or ndims entries.  Every column's filter is exact: one
        that could reach 2^31 in magnitude is a ValueError (rowops.fir_taps).  Rows in front of row 0 come from prev -- [T - 1, ndims], the last
        rows of the batch before this one, its last row being row -1 -- so that a stream continued over batches filters exactly; without prev
        they equal row 0 (edge replication: a smoothing filter has no start-up transient).  scipy.signal.lfilter's zero initial state is a prev
        of zeros.

            smooth = codec.fir_rows(batch, [1, 2, 1], dtype=torch.float32, scale=0.25)        # binomial smoothing
            season = codec.fir_rows(batch, [1] + [0] * 23 + [-1])                             # x[g] - x[g - 24]: diff(periods=24)
            second = codec.fir_rows(batch, [1, -2, 1])                                        # second difference

        dtype: None or torch.int32 for the sums themselves, or torch.float32 / torch.float16 / torch.bfloat16 for
        (y.to(float32) * scale[d] + offset[d]).to(dtype), bit for bit what torch computes on the CPU; scale / offset: float_rows' forms, a float
        dtype only.
        -> a [G, ndims] tensor, G = total_len / ndims; of a batch that ends mid-row the flat view of its total_len elements, as rolling_rows
        places them.  return_tail=True: -> (result, tail), tail the batch's last T - 1 raw rows [T - 1, ndims] (read_rows; completed from prev,
        or by row 0, where the batch is shorter): the prev of the next batch.  out: a contiguous tensor of the output dtype with at least
        nchunks x chunk_len elements to write into; rets: an int64 tensor of nchunks entries for the per-chunk element counts.  One library
        call: the decode and, with more than one tap, its seam pass.  A damaged chunk's rows are unspecified, and the first T - 1 rows of the
        chunk behind it; check=True raises SprintzError naming the first damaged chunk."""
        torch = self.torch
        D, n = self.ndims, batch.nchunks
        R, _ = rowops.chunk_rows(self.chunk_len, D, "fir_rows")
        t, b = rowops.fir_taps(taps, bias, D, self.esz, self.device)
        T = int(t.shape[0])
        if T - 1 > R:
            raise ValueError(f"{T} taps reach {T - 1} rows back, more than the {R} rows of a chunk: a filter may reach into one chunk in front, not two")
        if dtype is None or dtype == torch.int32:
            if scale is not None or offset is not None:
                raise ValueError("scale and offset go with a float dtype")
            dtype, fmt = torch.int32, _lib.DERIVE_I32
        else:
            fmt = 1 + rowops.float_format(dtype)
            scale = rowops.float_params(scale, D, "scale", self.device)
            offset = rowops.float_params(offset, D, "offset", self.device)
        if prev is not None and T > 1:
            if not torch.is_tensor(prev):
                prev = np.asarray(prev).reshape(-1).tolist()
            prev = rowops.elem_tensor(prev, (T - 1) * D, self.esz, self.dtype, self.device, "prev").view(T - 1, D)
        else:
            prev = None
        if out is None:
            out = torch.empty(max(n * self.chunk_len, 1), dtype=dtype, device=self.device)
        elif not torch.is_tensor(out) or out.dtype != dtype or out.device != self.device or out.numel() < n * self.chunk_len or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous {dtype} tensor of at least {n} x {self.chunk_len} elements on {self.device}")
        if rets is None:
            rets = self._rets(n, check)
        tmp = torch.empty(max(rowops.fir_tmp_bytes(n, T, D, self.esz) // 16, 1) * 2, dtype=torch.int64, device=self.device) if T > 1 else None
        if n:
            with self._on():
                _lib.check(_lib.fir_rows(_CODEC_ID[self.codec], self.esz, batch.data.data_ptr(), batch.offsets.data_ptr(), n, self.chunk_len, D, T,
                                         t.data_ptr(), b.data_ptr(), fmt, _ptr(scale), _ptr(offset), _ptr(prev), self._general(general_layout),
                                         _ptr(tmp), out.data_ptr(), _ptr(rets), self._stream()))
            if check:
                rowops.raise_damaged("fir_rows", rets, n, _lib.SprintzError)
        res = out.view(-1)[: batch.total_len]
        res = res.view(-1, D) if batch.total_len % D == 0 else res
        if not return_tail:
            return res
        G = batch.total_len // D
        have = min(G, T - 1)
        tail = self.read_rows(batch, G - have, G) if have else torch.empty((0, D), dtype=self.dtype, device=self.device)
        if have < T - 1:
            if prev is not None:
                front = prev[have:]
            elif G:
                front = self.read_rows(batch, 0, 1).expand(T - 1 - have, D)
            else:
                raise ValueError("return_tail of a batch without a row needs prev")
            sv = torch.int8 if self.esz == 1 else torch.int16                   # (through the signed type of the same width, as elem_tensor goes)
            tail = torch.cat([front.view(sv), tail.view(sv)]).view(self.dtype).contiguous()
        return res, tail

    def _fir_own_taps(self, name, kw):
        if "taps" in kw:
            raise ValueError(f"{name} builds taps itself")

    def shift_rows(self, batch, k, **kw):
        """pandas' shift(k) with the edge replicated: out[g, d] = x[g - k, d] as int32 (fir_rows with a unit tap at lag k; the first k rows hold
        row 0, or the rows prev gives).  Every other argument is fir_rows'."""
        self._fir_own_taps("shift_rows", kw)
        return self.fir_rows(batch, rowops.shift_taps(k), **kw)

    def lag_diff_rows(self, batch, periods=1, **kw):
        """pandas' diff(periods): out[g, d] = x[g, d] - x[g - periods, d] as int32, the seasonal difference (fir_rows with +1 at lag 0 and -1 at
        lag periods; the first `periods` rows change against row 0, or against the rows prev gives).  Every other argument is fir_rows'."""
        self._fir_own_taps("lag_diff_rows", kw)
        return self.fir_rows(batch, rowops.lag_diff_taps(periods), **kw)

    def smooth_rows(self, batch, taps, dtype=None, **kw):
        """A smoothing filter: fir_rows with a float dtype (float32 unless given) and scale = 1 / sum(taps), so that taps of any positive sum
        average -- [1, 2, 1] is the binomial, [1, 2, 3, 2, 1] a triangular window.  taps: T integers shared by all columns.  Every other argument
        is fir_rows'; scale is this wrapper's."""
        if "scale" in kw:
            raise ValueError("smooth_rows builds scale itself")
        dtype = self.torch.float32 if dtype is None else dtype
        if dtype == self.torch.int32:
            raise ValueError("smooth_rows needs a float dtype")
        vals = taps.tolist() if self.torch.is_tensor(taps) or isinstance(taps, np.ndarray) else taps
        if np.isscalar(vals) or isinstance(vals, dict) or vals is None or not all(np.isscalar(e) for e in vals):
            raise ValueError("smooth_rows takes 1-D taps, T integers shared by all columns: per-column taps have no one sum to scale by (use fir_rows with scale)")
        total = sum(int(e) for e in vals)
        if total <= 0:
            raise ValueError(f"smooth_rows needs taps of a positive sum, not {total}")
        return self.fir_rows(batch, taps, dtype=dtype, scale=1.0 / total, **kw)

    def cumulative_rows(self, batch, ops=("min", "max", "sum"), sum_dtype=None, carry=None, return_carry=False, general_layout=False, check=True):
        """Running min / max / sum / mean of every column from the first row on, one result per row -- cummin, cummax, cumsum and pandas'
        expanding().mean() -- straight from the compressed batch: the decoded tensor never exists.  Batch row g is row g % R of chunk g // R,
        R = chunk_len / ndims (chunk_len must be a multiple of ndims), and out[g, d] = op(seed[d], x[0 .. g, d]).

        ops: any of "min", "max" (the codec's dtype, unsigned), "sum" (sum_dtype: torch.int64, the default, exact modulo 2^64, or torch.int32,
        its low half) and "mean" (float64: the int64 sum over the rows so far; it needs int64 sums).  carry: what an earlier call returned
        with return_carry=True -- the stream goes on where that batch ended, as if the two were one; None: a fresh start.
        -> {op: [G, ndims]}, G = ceil(total_len / ndims); the columns a partial last row lacks hold 0.  With return_carry=True -> (that, carry).
        One library call: with more than one chunk the chunks' totals, their scan and the decode.  A damaged chunk counts as no rows for
        everything behind it; check=True raises SprintzError naming the first one."""
        torch = self.torch
        ops = rowops.normalise_ops(ops, rowops.CUMULATIVE_OPS, '"min", "max", "sum", "mean"')
        sum_dtype = torch.int64 if sum_dtype is None else sum_dtype
        if sum_dtype not in (torch.int64, torch.int32):
            raise ValueError(f"sum_dtype must be torch.int64 or torch.int32, not {sum_dtype}")
        if "mean" in ops and sum_dtype != torch.int64:
            raise ValueError('"mean" needs int64 sums: sum_dtype=torch.int32 keeps only the low half')
        D, n = self.ndims, batch.nchunks
        rowops.chunk_rows(self.chunk_len, D, "cumulative_rows")
        G = -(-batch.total_len // D)
        cin = None if carry is None else rowops.check_carry(carry, D, self.device)
        cout = rowops.CumulativeCarry(torch.empty((3, D), dtype=torch.int64, device=self.device), (cin.rows if cin else 0) + G) if return_carry else None
        want_sum = "sum" in ops or "mean" in ops
        bits = (_lib.CUM_MIN if "min" in ops else 0) | (_lib.CUM_MAX if "max" in ops else 0) | (_lib.CUM_SUM if want_sum else 0)
        raw = {}
        for name, dt in (("min", self.dtype), ("max", self.dtype), ("sum", sum_dtype)):
            if name in ops or (name == "sum" and want_sum):
                raw[name] = torch.empty(max(n * self.chunk_len, 1), dtype=dt, device=self.device)
        tmp = torch.empty(max(rowops.cumulative_tmp_bytes(n, D) // 16, 1) * 2, dtype=torch.int64, device=self.device)
        rets = self._rets(n, check)
        with self._on():
            _lib.check(_lib.cumulative_rows(_CODEC_ID[self.codec], self.esz, batch.data.data_ptr(), batch.offsets.data_ptr(), n, self.chunk_len, D,
                                            bits, 8 if sum_dtype == torch.int64 else 4, self._general(general_layout),
                                            _ptr(raw.get("min")), _ptr(raw.get("max")), _ptr(raw.get("sum")),
                                            _ptr(cin.table if cin else None), _ptr(cout.table if cout else None), tmp.data_ptr(), _ptr(rets), self._stream()))
        if check and n:
            rowops.raise_damaged("cumulative_rows", rets, n, _lib.SprintzError)
        res = {}
        for name, v in raw.items():
            v = v[: G * D]
            v[batch.total_len:] = 0
            res[name] = v.view(G, D)
        if "mean" in ops:
            res["mean"] = rowops.cumulative_mean(res["sum"], cin.rows if cin else 0)
            if batch.total_len < G * D:
                res["mean"].view(-1)[batch.total_len:] = 0
        res = {k: res[k] for k in ops}
        return (res, cout) if return_carry else res

    def where(self, batch, lo, hi, mode="all", ids=False, general_layout=False, zones=None):
        """SELECT * WHERE: the rows that satisfy the bounds (filter_rows' lo / hi / mode), straight from the compressed batch -- the
        filter launch, a prefix sum of its counts and the select launch; the batch is never materialised.
        -> {"rows": [total, ndims], and with ids=True "ids": int64 [total]}, in ascending batch row order.
        zones: the batch's ZoneMap (zone_map) for the filter step -- that half alone is pruned, the select launch decodes every chunk."""
        return self._where("where", self.select_rows, batch, lo, hi, mode, counts=True, ids=ids, general_layout=general_layout, zones=zones)

    def aggregate_rows(self, batch, mask, window_rows=None, ops=("count", "min", "max", "sum"), general_layout=False, per_chunk=False,
                       check=True):
        """Per-window min / max / sum / count of the rows a mask names, fused into the decode (one launch; only the results leave the chip).

        mask: uint8 [nchunks, MB] in filter_rows' layout (MB = ceil(R / 8), R = chunk_len / ndims: chunk_len must be a multiple of
        ndims) -- from filter_rows on this batch, several masks combined, or another batch on the same time base; bits of rows that do
        not exist are ignored.  window_rows=None: one window a chunk.
        per_chunk=True: the kernel's chunk-relative windows, {op: [nchunks, nwin, ndims]} and "count": [nchunks, nwin], nwin =
        ceil(R / window_rows), window_rows a multiple of 8.  Default: windows over the batch's rows, as query_windows folds them --
        {op: [nwindows, ndims]}, "count": [nwindows] -- which needs R to be a multiple of window_rows or a divisor of it.
        ops: any of "min", "max" (codec dtype), "sum", "count" (int64) and "mean" (float64: sum / count, NaN where count is 0).  A window
        with no selected row holds the identities (min all ones, max 0, sum 0, count 0).  check=True raises SprintzError naming the
        first damaged chunk."""
        torch = self.torch
        ops = rowops.normalise_ops(ops, ("min", "max", "sum", "count", "mean"), "min / max / sum / count / mean")
        D, n = self.ndims, batch.nchunks
        R, MB = rowops.chunk_rows(self.chunk_len, D, "aggregate_rows")
        mask = rowops.check_mask(mask, n, MB, self.device)
        kw, fold, nwin = rowops.plan_windows(R, window_rows, per_chunk)
        want = set(ops) | ({"sum", "count"} if "mean" in ops else set())
        bits = (_lib.AGG_MIN if "min" in want else 0) | (_lib.AGG_MAX if "max" in want else 0) | (_lib.AGG_SUM if "sum" in want else 0) | \
               (_lib.AGG_COUNT if "count" in want else 0)
        res = {}
        if bits & _lib.AGG_MIN:
            res["min"] = torch.empty((n, nwin, D), dtype=self.dtype, device=self.device)
        if bits & _lib.AGG_MAX:
            res["max"] = torch.empty((n, nwin, D), dtype=self.dtype, device=self.device)
        if bits & _lib.AGG_SUM:
            res["sum"] = torch.empty((n, nwin, D), dtype=torch.int64, device=self.device)
        cnt32 = torch.empty((n, nwin), dtype=torch.int32, device=self.device) if bits & _lib.AGG_COUNT else None
        rets = self._rets(n, check)
        with self._on():
            _lib.check(_lib.aggregate_rows(_CODEC_ID[self.codec], self.esz, batch.data.data_ptr(), batch.offsets.data_ptr(), n,
                                           self.chunk_len, D, mask.data_ptr(), kw, bits, self._general(general_layout),
                                           res["min"].data_ptr() if "min" in res else None,
                                           res["max"].data_ptr() if "max" in res else None,
                                           res["sum"].data_ptr() if "sum" in res else None,
                                           cnt32.data_ptr() if cnt32 is not None else None,
                                           rets.data_ptr() if rets is not None else None, self._stream()))
        if check:
            rowops.raise_damaged("aggregate_rows", rets, n, _lib.SprintzError)
        if cnt32 is not None:
            res["count"] = cnt32.to(torch.int64)
        out = res
        if not per_chunk:
            W = R if window_rows is None else int(window_rows)
            out = rowops.fold_windows(res, n, nwin, D, W, fold, batch.total_len, self.esz, self.dtype)
        if "mean" in ops:                                   # 0 / 0 is NaN: a window with no selected row has no mean
            out["mean"] = out["sum"].to(torch.float64) / out["count"].to(torch.float64).unsqueeze(-1)
        return {k: v for k, v in out.items() if k in ops}

    def aggregate_where(self, batch, lo, hi, mode="all", window_rows=None, ops=("count", "min", "max", "sum"), general_layout=False, zones=None):
        """SELECT count(*), min(x), max(x), sum(x) WHERE <bounds> [GROUP BY window]: filter_rows (its lo / hi / mode) and aggregate_rows
        on its mask -- two decode-speed launches; the batch is never materialised.  -> aggregate_rows' global windows.
        zones: the batch's ZoneMap (zone_map) for the filter step -- that half alone is pruned, the aggregate launch decodes every chunk."""
        return self._where("aggregate_where", self.aggregate_rows, batch, lo, hi, mode, window_rows=window_rows, ops=ops,
                           general_layout=general_layout, zones=zones)

    def histogram_rows(self, batch, mask=None, nbins=256, lo=None, shift=None, chunks_per_hist=0, general_layout=False, check=True):
        """Per-column value counts of the rows a mask names, fused into the decode (one launch; only the counts leave the chip).

        mask: uint8 [nchunks, MB] in filter_rows' layout (MB = ceil(R / 8), R = chunk_len / ndims: chunk_len must be a multiple of
        ndims), or None: every row; bits of rows that do not exist are ignored.
        A value x of column d is counted in bin ((x - lo[d]) mod 2^W) >> shift if that is below nbins, and dropped otherwise.  lo: a
        scalar, ndims entries or a tensor; None: 0.  shift=None: the one that makes nbins bins cover the element range,
        W - ceil(log2(nbins)) (W - 1 for one bin).  ndims * nbins is at most 16384 a call: split wider requests with lo.
        chunks_per_hist = H: chunks [g H, (g + 1) H) share histogram g; 0: one histogram for the batch.
        -> int64 [ngroups, ndims, nbins].  check=True raises SprintzError naming the first damaged chunk."""
        torch = self.torch
        D, n, W = self.ndims, batch.nchunks, 8 * self.esz
        R, MB = rowops.chunk_rows(self.chunk_len, D, "histogram_rows")
        nbins, H = int(nbins), int(chunks_per_hist)
        if nbins < 1 or H < 0:
            raise ValueError("nbins must be positive and chunks_per_hist must not be negative")
        shift = rowops.default_shift(W, nbins) if shift is None else int(shift)
        if mask is not None:
            mask = rowops.check_mask(mask, n, MB, self.device)
        lo_t = None if lo is None else rowops.elem_tensor(lo, D, self.esz, self.dtype, self.device, "lo")
        ngroups = -(-n // H) if H else 1
        hist = torch.empty((ngroups if n else 0, D, nbins), dtype=torch.int64, device=self.device)
        if n == 0:
            return hist
        rets = self._rets(n, check)
        with self._on():
            _lib.check(_lib.histogram_rows(_CODEC_ID[self.codec], self.esz, batch.data.data_ptr(), batch.offsets.data_ptr(), n,
                                           self.chunk_len, D, mask.data_ptr() if mask is not None else None,
                                           lo_t.data_ptr() if lo_t is not None else None, shift, nbins, H, self._general(general_layout),
                                           hist.data_ptr(), rets.data_ptr() if rets is not None else None, self._stream()))
        if check:
            rowops.raise_damaged("histogram_rows", rets, n, _lib.SprintzError)
        return hist

    def histogram_where(self, batch, lo, hi, mode="all", **kw):
        """The distribution of the rows that satisfy a condition: filter_rows (its lo / hi / mode) and histogram_rows on its mask -- two
        decode-speed launches; the batch is never materialised.  kw: histogram_rows' other arguments (nbins, its own lo as hist_lo,
        shift, chunks_per_hist, general_layout) and zones, the batch's ZoneMap (zone_map) for the filter step -- that half alone is pruned."""
        if "hist_lo" in kw:
            kw["lo"] = kw.pop("hist_lo")
        return self._where("histogram_where", self.histogram_rows, batch, lo, hi, mode, **kw)

    def _hist_span(self, batch, mask, shift, total_bins, lo64=None):
        """one histogram of the batch, total_bins bins of 2^shift values from lo64 [ndims] (int64 device tensor; None: 0) on, as int64
        [ndims, total_bins]: as many calls as the cap on ndims * nbins asks for, side by side"""
        torch = self.torch
        D, W = self.ndims, 8 * self.esz
        nb = total_bins
        while D * nb > _lib.HIST_MAX_COUNTERS:
            nb //= 2
        parts = []
        for k in range(total_bins // nb):
            if lo64 is None and k == 0:
                lo_k = None
            else:
                base = lo64 if lo64 is not None else torch.zeros(D, dtype=torch.int64, device=self.device)
                lo_k = (base + ((k * nb) << shift)) % (1 << W)
            parts.append(self.histogram_rows(batch, mask=mask, nbins=nb, lo=lo_k, shift=shift)[0])
        return parts[0] if len(parts) == 1 else torch.cat(parts, dim=1)

    def quantiles(self, batch, q, mask=None):
        """EXACT per-column quantiles of the whole batch (of the rows a mask names), straight from the compressed data: histogram
        passes and cumulative sums on the device, no sample leaves the chip.

        q: quantiles in [0, 1].  -> [len(q), ndims] of the codec's dtype: for a column with n selected values, the value at index
        max(ceil(q n), 1) - 1 of them sorted.  Raises ValueError where n == 0.
        8-bit data: one full-resolution pass.  16-bit data: a coarse pass (256 bins of 256 values), then one refinement pass (256
        bins of one value, lo at the start of the wanted coarse bin, column by column) for each group of quantiles that fall in the
        same coarse bin of their column.  Passes are split with lo where ndims * 256 exceeds a call's counters."""
        torch = self.torch
        D, W = self.ndims, 8 * self.esz
        qs = [float(x) for x in (q if np.ndim(q) else [q])]
        if not qs or any(not 0.0 <= x <= 1.0 for x in qs):
            raise ValueError("q must be one or more numbers in [0, 1]")
        if batch.nchunks == 0:
            raise ValueError("quantiles of an empty batch")
        Q = len(qs)
        coarse = self._hist_span(batch, mask, W - 8, 256)                        # [D, 256]
        cum = torch.cumsum(coarse, dim=1)
        n = cum[:, -1]
        if bool((n == 0).any().item()):
            raise ValueError("quantiles: no row is selected")
        qt = torch.tensor(qs, dtype=torch.float64, device=self.device)
        k = (torch.ceil(qt[None, :] * n[:, None].to(torch.float64)).to(torch.int64).clamp(min=1) - 1).contiguous()   # [D, Q]
        cb = torch.searchsorted(cum, k, right=True)                              # the first bin whose cumulative count exceeds the index
        if W == 8:
            return cb.t().contiguous().to(torch.uint8)
        k2 = k - (torch.gather(cum, 1, cb) - torch.gather(coarse, 1, cb))        # the index inside the coarse bin
        # the quantiles of a column that share a coarse bin share a pass: rank of each quantile's bin among its column's distinct bins
        scb, order = torch.sort(cb, dim=1)
        step = torch.zeros_like(scb)
        step[:, 1:] = (scb[:, 1:] != scb[:, :-1]).to(torch.int64)
        rank = torch.empty_like(cb).scatter_(1, order, torch.cumsum(step, dim=1))
        out = torch.zeros_like(cb)
        for j in range(int(rank.max().item()) + 1):
            here = rank == j
            bin_j = torch.where(here, cb, torch.zeros_like(cb)).amax(dim=1)      # [D]: the column's j-th distinct bin (0 where it has fewer)
            fine = self._hist_span(batch, mask, 0, 256, lo64=bin_j << 8)
            fb = torch.searchsorted(torch.cumsum(fine, dim=1), k2, right=True)
            out = torch.where(here, (cb << 8) + fb, out)
        half = 1 << 15
        return (((out.t().contiguous() + half) % (1 << 16)) - half).to(torch.int16).view(torch.uint16)

    _MOM_INT = ("count", "sum", "sumsq", "cross")
    _MOM_DERIVED = ("mean", "var", "std", "cov", "corr")

    def moments_rows(self, batch, mask=None, window_rows=None, ref=None, ops=("count", "sum", "sumsq"), general_layout=False, per_chunk=False,
                     check=True, ddof=0):
        """Per-window count, sum, sum of squares and sum of products with the column `ref` of the rows a mask names -- and the mean,
        variance, standard deviation, covariance and correlation that follow from them -- fused into the decode (one launch; only the
        results leave the chip).

        mask, window_rows, general_layout, per_chunk, check: as in aggregate_rows, except that mask=None means every existing row.
        per_chunk=True: the kernel's chunk-relative windows, {op: [nchunks, nwin, ndims]} and "count": [nchunks, nwin]; default: windows
        over the batch's rows, {op: [nwindows, ndims]}, "count": [nwindows], which needs the chunk's rows to be a multiple or a divisor
        of window_rows.
        ops: any of the exact integer sums "count" (n), "sum" (S = sum x), "sumsq" (Q = sum x^2), "cross" (P = sum x * x_ref) -- int64 --
        and of the derived "mean", "var", "std", "cov" (with x_ref), "corr" (with x_ref) -- float64.  "cross", "cov" and "corr" need
        ref.  ddof (0 or 1) divides var / std / cov by n - ddof.  A window with no selected row holds zeros; derived values are NaN
        where n == 0 or n <= ddof, and corr also where either variance is 0.

        Derived values rest on an integer pivot, not on n Q - S^2 in float64, which cancels: rowops.derive_moments.
        check=True raises SprintzError naming the first damaged chunk."""
        torch = self.torch
        ops = rowops.normalise_ops(ops, self._MOM_INT + self._MOM_DERIVED, "count / sum / sumsq / cross / mean / var / std / cov / corr")
        if ddof not in (0, 1):
            raise ValueError("ddof must be 0 or 1")
        D, n = self.ndims, batch.nchunks
        if set(ops) & {"cross", "cov", "corr"}:
            if ref is None:
                raise ValueError('"cross", "cov" and "corr" need ref, the reference column')
            if not 0 <= int(ref) < D:
                raise ValueError(f"ref must be a column of the batch, 0 .. {D - 1}")
        R, MB = rowops.chunk_rows(self.chunk_len, D, "moments_rows")
        if mask is not None:
            mask = rowops.check_mask(mask, n, MB, self.device)
        kw, fold, nwin = rowops.plan_windows(R, window_rows, per_chunk)
        want = set(ops) & set(self._MOM_INT)
        if "mean" in ops:
            want |= {"count", "sum"}
        if set(ops) & {"var", "std"}:
            want |= {"count", "sum", "sumsq"}
        if "cov" in ops:
            want |= {"count", "sum", "cross"}
        if "corr" in ops:
            want |= {"count", "sum", "sumsq", "cross"}
        bits = (_lib.MOM_COUNT if "count" in want else 0) | (_lib.MOM_SUM if "sum" in want else 0) | (_lib.MOM_SUMSQ if "sumsq" in want else 0) | \
               (_lib.MOM_CROSS if "cross" in want else 0)
        res = {k: torch.empty((n, nwin, D), dtype=torch.int64, device=self.device) for k in ("sum", "sumsq", "cross") if k in want}
        cnt32 = torch.empty((n, nwin), dtype=torch.int32, device=self.device) if "count" in want else None
        rets = self._rets(n, check)
        with self._on():
            _lib.check(_lib.moments_rows(_CODEC_ID[self.codec], self.esz, batch.data.data_ptr(), batch.offsets.data_ptr(), n,
                                         self.chunk_len, D, mask.data_ptr() if mask is not None else None, kw, bits,
                                         int(ref) if "cross" in want else 0, self._general(general_layout),
                                         cnt32.data_ptr() if cnt32 is not None else None,
                                         res["sum"].data_ptr() if "sum" in res else None,
                                         res["sumsq"].data_ptr() if "sumsq" in res else None,
                                         res["cross"].data_ptr() if "cross" in res else None,
                                         rets.data_ptr() if rets is not None else None, self._stream()))
        if check:
            rowops.raise_damaged("moments_rows", rets, n, _lib.SprintzError)
        if cnt32 is not None:
            res["count"] = cnt32.to(torch.int64)
        out = res
        if not per_chunk:
            W = R if window_rows is None else int(window_rows)
            out = rowops.fold_windows(res, n, nwin, D, W, fold, batch.total_len, self.esz, self.dtype)
        if set(ops) & set(self._MOM_DERIVED):
            out.update(rowops.derive_moments(out, ops, ref, ddof))
        return {k: v for k, v in out.items() if k in ops}

    def moments_where(self, batch, lo, hi, mode="all", **kw):
        """SELECT count(*), sum(x), var(x), corr(x, y), ... WHERE <bounds> [GROUP BY window]: filter_rows (its lo / hi / mode) and
        moments_rows on its mask -- two decode-speed launches; the batch is never materialised.  kw: moments_rows' other arguments, and zones, the batch's
        ZoneMap (zone_map) for the filter step -- that half alone is pruned."""
        return self._where("moments_where", self.moments_rows, batch, lo, hi, mode, **kw)

    _EXT_OPS = ("min", "max", "argmin", "argmax", "first", "last", "rows", "count")

    def extrema_rows(self, batch, mask=None, window_rows=None, ops=("min", "argmin", "max", "argmax"), general_layout=False, per_chunk=False,
                     check=True):
        """Per-window min / max of the rows a mask names WITH the rows they stand in, and the window's first and last selected sample, fused
        into the decode (one launch; only the results leave the chip): "when did the peak happen?".

        mask, window_rows, general_layout, per_chunk, check: as in aggregate_rows, except that mask=None means every existing row.
        per_chunk=True: the kernel's chunk-relative windows, {op: [nchunks, nwin, ndims]}; default: windows over the batch's rows,
        {op: [nwindows, ndims]}, which needs the chunk's rows to be a multiple or a divisor of window_rows.
        ops: any of "min", "max" (codec dtype); "argmin", "argmax" (int64: the BATCH row, chunk * R + row, of the FIRST selected row that
        holds the minimum / maximum -- numpy's tie rule; -1 where the window has no selected row); "first", "last" (codec dtype: the
        column's value in the window's first / last selected row, 0 where there is none); "rows" (returned as "first_row" and "last_row":
        int64 [...] batch rows of those two rows, -1 where there is none); "count" (int64 [...]).  A window with no selected row holds min
        all ones and max 0.  check=True raises SprintzError naming the first damaged chunk."""
        torch = self.torch
        ops = rowops.normalise_ops(ops, self._EXT_OPS, "min / max / argmin / argmax / first / last / rows / count")
        D, n = self.ndims, batch.nchunks
        R, MB = rowops.chunk_rows(self.chunk_len, D, "extrema_rows")
        if mask is not None:
            mask = rowops.check_mask(mask, n, MB, self.device)
        kw, fold, nwin = rowops.plan_windows(R, window_rows, per_chunk)
        want = set(ops)
        if fold > 1:                                        # what the fold compares: the values beside their rows, the rows beside first / last
            want |= ({"min"} if "argmin" in want else set()) | ({"max"} if "argmax" in want else set()) | ({"rows"} if want & {"first", "last"} else set())
        bit = dict(zip(self._EXT_OPS, (_lib.EXT_MIN, _lib.EXT_MAX, _lib.EXT_ARGMIN, _lib.EXT_ARGMAX, _lib.EXT_FIRST, _lib.EXT_LAST, _lib.EXT_ROWS, _lib.EXT_COUNT)))
        bits = sum(bit[k] for k in want)
        raw = {k: torch.empty((n, nwin, D), dtype=self.dtype, device=self.device) for k in ("min", "max", "first", "last") if k in want}
        raw.update({k: torch.empty((n, nwin, D), dtype=torch.int32, device=self.device) for k in ("argmin", "argmax") if k in want})
        if "rows" in want:
            raw["rows"] = torch.empty((n, nwin, 2), dtype=torch.int32, device=self.device)
        if "count" in want:
            raw["count"] = torch.empty((n, nwin), dtype=torch.int32, device=self.device)
        rets = self._rets(n, check)
        ptr = lambda k: raw[k].data_ptr() if k in raw else None
        with self._on():
            _lib.check(_lib.extrema_rows(_CODEC_ID[self.codec], self.esz, batch.data.data_ptr(), batch.offsets.data_ptr(), n,
                                         self.chunk_len, D, mask.data_ptr() if mask is not None else None, kw, bits, self._general(general_layout),
                                         ptr("min"), ptr("max"), ptr("argmin"), ptr("argmax"), ptr("first"), ptr("last"), ptr("rows"), ptr("count"),
                                         rets.data_ptr() if rets is not None else None, self._stream()))
        if check:
            rowops.raise_damaged("extrema_rows", rets, n, _lib.SprintzError)
        # chunk-relative uint32 rows (all ones: none) -> int64 batch rows (-1: none)
        base = (torch.arange(n, dtype=torch.int64, device=self.device) * R).reshape(n, 1, 1)

        def batch_rows(v):
            v = v.to(torch.int64)                           # int32 -1 is SPRINTZ_EXT_NO_ROW
            return torch.where(v >= 0, v + base, v)

        res = {k: v for k, v in raw.items() if k in ("min", "max", "first", "last")}
        for k in ("argmin", "argmax"):
            if k in raw:
                res[k] = batch_rows(raw[k])
        if "rows" in raw:
            fl = batch_rows(raw["rows"])
            res["first_row"], res["last_row"] = fl[..., 0], fl[..., 1]
        if "count" in raw:
            res["count"] = raw["count"].to(torch.int64)
        out = res
        if not per_chunk:
            W = R if window_rows is None else int(window_rows)
            out = rowops.fold_extrema(res, n, nwin, D, W, fold, batch.total_len, self.esz, self.dtype)
        keep = set(ops) - {"rows"} | ({"first_row", "last_row"} if "rows" in ops else set())
        return {k: v for k, v in out.items() if k in keep}

    def extrema_where(self, batch, lo, hi, mode="all", **kw):
        """SELECT min(x), argmin(x), max(x), argmax(x), ... WHERE <bounds> [GROUP BY window]: filter_rows (its lo / hi / mode) and
        extrema_rows on its mask -- two decode-speed launches; the batch is never materialised.  kw: extrema_rows' other arguments, and zones, the batch's
        ZoneMap (zone_map) for the filter step -- that half alone is pruned."""
        return self._where("extrema_where", self.extrema_rows, batch, lo, hi, mode, **kw)

    def m4(self, batch, window_rows, mask=None):
        """The M4 reduction of the batch: per window of window_rows batch rows (a pixel column of a line chart) the first, the last, the
        minimum and the maximum sample with their time stamps -- the loss-free downsampling for line charts -- in one extrema_rows launch.
        -> {"t_first", "t_last": int64 [nw] batch rows; "v_first", "v_last", "v_min", "v_max": [nw, ndims] of the codec's dtype; "t_min",
        "t_max": int64 [nw, ndims]}; a time stamp is -1 where the window has no (selected) row.  Window rules: extrema_rows' global windows."""
        e = self.extrema_rows(batch, mask=mask, window_rows=window_rows, ops=("min", "argmin", "max", "argmax", "first", "last", "rows"))
        return {"t_first": e["first_row"], "v_first": e["first"], "t_min": e["argmin"], "v_min": e["min"],
                "t_max": e["argmax"], "v_max": e["max"], "t_last": e["last_row"], "v_last": e["last"]}

    _SEG_OPS = ("min", "max", "sum")

    def segment_rows(self, batch, mask, mode="runs", ops=("min", "max", "sum"), min_rows=1, general_layout=False, check=True):
        """A row mask's own structure, fused into the decode: per segment its first batch row, its length and the min / max / sum of every
        column over it -- a few bytes a segment leave the chip.

        mask: uint8 [nchunks, MB] in filter_rows' layout (MB = ceil(R / 8), R = chunk_len / ndims: chunk_len must be a multiple of
        ndims); bits of rows that do not exist are ignored, whatever they hold.
        mode="runs": the segments are the maximal runs of selected rows -- event detection: for each excursion, when it started, how
        long it lasted, its peak ("max") and its integral ("sum").  mode="splits": every row belongs to a segment and a set bit opens a new
        one -- sessionisation: the mask is a change log (sessions).
        The kernel's segments are relative to the chunk; they are stitched over the chunk seams here (rowops.fold_segments), so the result
        is what one chunk holding the whole batch would give.  Then segments shorter than min_rows are dropped.
        -> {"start": int64 [S] batch rows, "rows": int64 [S], and the selected ops: "min", "max" [S, ndims] of the codec's dtype, "sum"
        int64 [S, ndims]}, in ascending batch row order.  The call is segment_count (with the lengths total_len gives), a prefix sum, one
        read of the total, segment_rows and the fold.  check=True raises SprintzError naming the first damaged chunk."""
        torch = self.torch
        if mode not in rowops.SEGMENT_MODES:
            raise ValueError("mode must be 'runs' or 'splits'")
        ops = rowops.normalise_ops(ops, self._SEG_OPS, "min / max / sum") if ops else ()
        D, n = self.ndims, batch.nchunks
        R, MB = rowops.chunk_rows(self.chunk_len, D, "segment_rows")
        mask = rowops.check_mask(mask, n, MB, self.device)
        seg_mode = _lib.SEG_RUNS if mode == "runs" else _lib.SEG_SPLITS
        i64 = dict(dtype=torch.int64, device=self.device)
        lens = (batch.total_len - torch.arange(n, **i64) * self.chunk_len).clamp(min=0, max=self.chunk_len)
        counts = torch.zeros(n, dtype=torch.int32, device=self.device)
        with self._on():
            _lib.check(_lib.segment_count(mask.data_ptr(), n, self.chunk_len, D, seg_mode, lens.data_ptr(), counts.data_ptr(), self._stream()))
        counts = counts.to(torch.int64)
        incl = torch.cumsum(counts, 0)
        total = int(incl[-1].item()) if n else 0
        raw = {"start": torch.zeros(total, **i64), "rows32": torch.zeros(total, dtype=torch.int32, device=self.device)}
        raw.update({k: torch.empty((total, D), dtype=self.dtype, device=self.device) for k in ("min", "max") if k in ops})
        if "sum" in ops:
            raw["sum"] = torch.empty((total, D), **i64)
        if n:
            bits = _lib.SEG_ROWS | _lib.SEG_START | (_lib.SEG_MIN if "min" in ops else 0) | (_lib.SEG_MAX if "max" in ops else 0) | \
                   (_lib.SEG_SUM if "sum" in ops else 0)
            bases = (incl - counts).contiguous()
            rets = self._rets(n, check)
            # (no segment at all: the chunks are still checked, and a selected output must be there)
            hold = {k: v if v.numel() else v.new_empty(D) for k, v in raw.items()}
            ptr = lambda k: hold[k].data_ptr() if k in hold else None
            with self._on():
                _lib.check(_lib.segment_rows(_CODEC_ID[self.codec], self.esz, batch.data.data_ptr(), batch.offsets.data_ptr(), n,
                                             self.chunk_len, D, mask.data_ptr(), seg_mode, bases.data_ptr(), total, bits,
                                             self._general(general_layout), ptr("min"), ptr("max"), ptr("sum"), ptr("rows32"), ptr("start"),
                                             rets.data_ptr() if rets is not None else None, self._stream()))
            if check:
                rowops.raise_damaged("segment_rows", rets, n, _lib.SprintzError)
        raw["rows"] = raw.pop("rows32").to(torch.int64)
        return rowops.fold_segments(raw, mask.view(n, MB), R, mode, min_rows, self.dtype)

    def segments_where(self, batch, lo, hi, mode="all", **kw):
        """Event detection with event statistics: filter_rows (its lo / hi / mode) and segment_rows(mode="runs") on its mask -- for each
        excursion into the bounds its start, its length and the min / max / sum of every column over it; two decode-speed launches, the
        batch is never materialised.  kw: segment_rows' other arguments (ops, min_rows, general_layout, check), and zones, the batch's
        ZoneMap (zone_map) for the filter step -- that half alone is pruned."""
        seg = lambda b, mask, **k: self.segment_rows(b, mask, mode="runs", **k)      # noqa: E731
        return self._where("segments_where", seg, batch, lo, hi, mode, **kw)

    def sessions(self, batch, col, ops=("min", "max", "sum"), min_rows=1, general_layout=False, check=True):
        """Sessionisation on a state column: for each interval between two changes of column `col` its start, its duration ("rows") and
        the min / max / sum of every column over it.  filter_change on `col` marks the rows that do NOT change (x[g] == x[g - 1], over the
        chunk seams too), the mask is inverted in torch -- the change log; its padding bits and the bits of rows that do not exist come out
        set, which segment_rows ignores -- and segment_rows(mode="splits") cuts the batch at every set bit.  -> segment_rows' result."""
        same = self.filter_change(batch, col, lo=0, hi=0, general_layout=general_layout, check=check)["mask"]
        return self.segment_rows(batch, self.torch.bitwise_not(same), mode="splits", ops=ops, min_rows=min_rows, general_layout=general_layout,
                                 check=check)

    def groupby_rows(self, batch, key, nbins=256, key_lo=0, shift=None, mask=None, ops=("count", "sum"), chunks_per_table=0, general_layout=False,
                     check=True):
        """SELECT bin(x_key), count(*), sum(x_0), ..., sum(x_{D-1}) WHERE mask GROUP BY bin(x_key), fused into the decode (one launch; only
        the tables leave the chip): what conditional means rest on.

        key: the key column.  A row the mask names (mask: uint8 [nchunks, MB] in filter_rows' layout, MB = ceil(R / 8), R = chunk_len /
        ndims: chunk_len must be a multiple of ndims; None: every row; bits of rows that do not exist are ignored) whose key column holds
        x belongs to bin ((x - key_lo) mod 2^W) >> shift if that is below nbins, and is dropped otherwise.  shift=None: the one that
        makes nbins bins cover the element range, W - ceil(log2(nbins)) (W - 1 for one bin).  nbins * (ndims + 1) is at most 16384 a
        call: split wider requests with key_lo.
        chunks_per_table = H: chunks [t H, (t + 1) H) share table t; 0: one table for the batch.
        ops: "count", "sum" or both.  -> {"count": int64 [ntables, nbins], "sum": int64 [ntables, nbins, ndims]} and, where both are
        selected, "mean": float64 sum / count, NaN where count is 0.  check=True raises SprintzError naming the first damaged chunk."""
        torch = self.torch
        D, n, W = self.ndims, batch.nchunks, 8 * self.esz
        ops = rowops.normalise_ops(ops, ("count", "sum"), '"count" / "sum"')
        R, MB = rowops.chunk_rows(self.chunk_len, D, "groupby_rows")
        key, nbins, key_lo, H = int(key), int(nbins), int(key_lo), int(chunks_per_table)
        if not 0 <= key < D:
            raise ValueError(f"key must be a column of the batch, 0 .. {D - 1}")
        if nbins < 1 or H < 0:
            raise ValueError("nbins must be positive and chunks_per_table must not be negative")
        if not 0 <= key_lo < (1 << W):
            raise ValueError(f"key_lo must be in 0..{(1 << W) - 1}")
        shift = rowops.default_shift(W, nbins) if shift is None else int(shift)
        if mask is not None:
            mask = rowops.check_mask(mask, n, MB, self.device)
        ntables = (-(-n // H) if H else 1) if n else 0
        out = {}
        if "count" in ops:
            out["count"] = torch.empty((ntables, nbins), dtype=torch.int64, device=self.device)
        if "sum" in ops:
            out["sum"] = torch.empty((ntables, nbins, D), dtype=torch.int64, device=self.device)
        if n:
            rets = self._rets(n, check)
            with self._on():
                _lib.check(_lib.groupby_rows(_CODEC_ID[self.codec], self.esz, batch.data.data_ptr(), batch.offsets.data_ptr(), n,
                                             self.chunk_len, D, mask.data_ptr() if mask is not None else None, key, key_lo, shift, nbins, H,
                                             (_lib.GBY_COUNT if "count" in ops else 0) | (_lib.GBY_SUM if "sum" in ops else 0),
                                             self._general(general_layout),
                                             out["count"].data_ptr() if "count" in out else None,
                                             out["sum"].data_ptr() if "sum" in out else None,
                                             rets.data_ptr() if rets is not None else None, self._stream()))
            if check:
                rowops.raise_damaged("groupby_rows", rets, n, _lib.SprintzError)
        if "count" in out and "sum" in out:
            cnt = out["count"].unsqueeze(-1)
            nan = torch.full((), float("nan"), dtype=torch.float64, device=self.device)
            out["mean"] = torch.where(cnt > 0, out["sum"].to(torch.float64) / cnt.to(torch.float64), nan)
        return out

    def groupby_where(self, batch, lo, hi, mode="all", **kw):
        """SELECT bin(x_key), count(*), sum(x) WHERE <bounds> GROUP BY bin(x_key): filter_rows (its lo / hi / mode) and groupby_rows on its
        mask -- two decode-speed launches; the batch is never materialised.  kw: groupby_rows' other arguments (key among them), and zones, the
        batch's ZoneMap (zone_map) for the filter step -- that half alone is pruned."""
        return self._where("groupby_where", self.groupby_rows, batch, lo, hi, mode, **kw)

    def corr(self, batch, cols=None, mask=None, window_rows=None):
        """The correlation matrix of the columns `cols` (default: all) per window, straight from the compressed data: [nwindows,
        len(cols), len(cols)] float64, one moments_rows launch per reference column.  Symmetric, 1 on the diagonal; NaN where a window
        is empty or one of the two columns is constant in it."""
        torch = self.torch
        cols = list(range(self.ndims)) if cols is None else [int(c) for c in cols]
        if not cols or any(not 0 <= c < self.ndims for c in cols):
            raise ValueError(f"cols must be columns of the batch, 0 .. {self.ndims - 1}")
        idx = torch.tensor(cols, dtype=torch.int64, device=self.device)
        parts = [self.moments_rows(batch, mask=mask, window_rows=window_rows, ref=c, ops=("corr",))["corr"].index_select(-1, idx) for c in cols]
        return torch.stack(parts, dim=-1)

    def read_rows(self, batch, lo, hi):
        """batch rows [lo, hi) -> [hi - lo, ndims]: one range of gather_rows, its chunks decoded side by side in the same launch"""
        lo, hi = int(lo), int(hi)
        if not 0 <= lo < hi:
            raise ValueError("read_rows needs 0 <= lo < hi")
        return self.gather_rows(batch, [lo], hi - lo)[0]


# ---- query on compressed data, single call (the reference's names) -----------------------

class QueryTypes:                       # query.hpp:23-25
    NOOP, REDUCE_MAX, REDUCE_SUM = 0, 1, 2


@dataclass
class QueryParams:                      # query.hpp:27-30
    op: int = QueryTypes.NOOP
    materialize: bool = False


def _query(codec, esz, src, dest, qp, general):
    src = np.ascontiguousarray(src)
    ndims = int(src.view(np.uint8)[6]) | (int(src.view(np.uint8)[7]) << 8)
    result = np.zeros(max(ndims, 1), np.uint64)
    flags = _lib.QUERY_GENERAL_LAYOUT if general else 0
    ret = int(_lib.query[(codec, esz)](_np_ptr(src), _np_ptr(dest) if dest is not None else None, int(qp.op),
                                       int(bool(qp.materialize)), flags, _np_ptr(result)))
    return ret, result[:ndims]


def query_rowmajor_delta_rle_8b(src, dest, qp, general_layout=True):
    """sprintz_delta.h:95; returns (elements, per-column result).  general_layout=True is what the
    reference's *_rowmajor_*_rle_* streams use; pass False for streams made by sprintz_compress_*."""
    return _query("delta", 1, src, dest, qp, general_layout)


def query_rowmajor_delta_rle_16b(src, dest, qp, general_layout=True):
    return _query("delta", 2, src, dest, qp, general_layout)


def query_rowmajor_xff_rle_8b(src, dest, qp, general_layout=True):
    return _query("xff", 1, src, dest, qp, general_layout)


def query_rowmajor_xff_rle_16b(src, dest, qp, general_layout=True):
    return _query("xff", 2, src, dest, qp, general_layout)


# ---- non-RLE codecs, the reference's names (sprintz_delta.h:26-76) --------------------------------

def _c_norle(codec, esz, src, length, dest, ndims):
    src = np.ascontiguousarray(src)
    if src.dtype.itemsize != esz or src.size < length:
        raise ValueError("src dtype/size does not match the call")
    return int(_lib.compress_norle(codec, esz, _np_ptr(src), length, _np_ptr(dest), ndims))


def compress_rowmajor_8b(src, len, dest, ndims):  # noqa: A002
    return _c_norle(_lib.CODEC_BITPACK_NORLE, 1, src, len, dest, ndims)


def compress_rowmajor_16b(src, len, dest, ndims):  # noqa: A002
    return _c_norle(_lib.CODEC_BITPACK_NORLE, 2, src, len, dest, ndims)


def compress_rowmajor_delta_8b(src, len, dest, ndims):  # noqa: A002
    return _c_norle(_lib.CODEC_DELTA_NORLE, 1, src, len, dest, ndims)


def compress_rowmajor_delta_16b(src, len, dest, ndims):  # noqa: A002
    return _c_norle(_lib.CODEC_DELTA_NORLE, 2, src, len, dest, ndims)


def compress8b_rowmajor_xff(src, len, dest, ndims):  # noqa: A002 - sprintz_xff.h:28
    return _c_norle(_lib.CODEC_XFF_NORLE, 1, src, len, dest, ndims)


def decompress8b_rowmajor_xff(src, dest):
    return int(_lib.decompress_norle(_lib.CODEC_XFF_NORLE, 1, _np_ptr(np.ascontiguousarray(src)), _np_ptr(dest)))


def decompress_rowmajor_8b(src, dest):
    return int(_lib.decompress_norle(_lib.CODEC_BITPACK_NORLE, 1, _np_ptr(np.ascontiguousarray(src)), _np_ptr(dest)))


def decompress_rowmajor_16b(src, dest):
    return int(_lib.decompress_norle(_lib.CODEC_BITPACK_NORLE, 2, _np_ptr(np.ascontiguousarray(src)), _np_ptr(dest)))


def decompress_rowmajor_delta_8b(src, dest):
    return int(_lib.decompress_norle(_lib.CODEC_DELTA_NORLE, 1, _np_ptr(np.ascontiguousarray(src)), _np_ptr(dest)))


def decompress_rowmajor_delta_16b(src, dest):
    return int(_lib.decompress_norle(_lib.CODEC_DELTA_NORLE, 2, _np_ptr(np.ascontiguousarray(src)), _np_ptr(dest)))


# ---- stand-alone transforms (delta.h:17-68) -------------------------------------------------

def _enc_t(kind, esz, src, length, dest, ndims, write_size):
    src = np.ascontiguousarray(src)
    if src.dtype.itemsize != esz or src.size < length:
        raise ValueError("src dtype/size does not match the call")
    if dest.nbytes < length * esz + (6 if write_size else 0):
        raise ValueError("dest too small")
    return int(_lib.transform_encode(kind, esz, _np_ptr(src), length, _np_ptr(dest), ndims, int(bool(write_size))))


def _dec_t(kind, esz, src, dest, length=0, ndims=0):
    src = np.ascontiguousarray(src)
    return int(_lib.transform_decode(kind, esz, _np_ptr(src), _np_ptr(dest), length, ndims))


def encode_delta_rowmajor_8b(src, len, dest, ndims, write_size=True):  # noqa: A002 - reference's name (delta.h:17)
    return _enc_t(_lib.TRANSFORM_DELTA, 1, src, len, dest, ndims, write_size)


def encode_delta_rowmajor_16b(src, len, dest, ndims, write_size=True):  # noqa: A002 (delta.h:53)
    return _enc_t(_lib.TRANSFORM_DELTA, 2, src, len, dest, ndims, write_size)


def encode_doubledelta_rowmajor_8b(src, len, dest, ndims, write_size=True):  # noqa: A002 (delta.h:36)
    return _enc_t(_lib.TRANSFORM_DOUBLEDELTA, 1, src, len, dest, ndims, write_size)


def encode_doubledelta_rowmajor_16b(src, len, dest, ndims, write_size=True):  # noqa: A002 (delta.h:63)
    return _enc_t(_lib.TRANSFORM_DOUBLEDELTA, 2, src, len, dest, ndims, write_size)


def decode_delta_rowmajor_8b(src, dest, len=0, ndims=0):  # noqa: A002 - both reference forms (delta.h:19-24)
    return _dec_t(_lib.TRANSFORM_DELTA, 1, src, dest, len, ndims)


def decode_delta_rowmajor_16b(src, dest, len=0, ndims=0):  # noqa: A002
    return _dec_t(_lib.TRANSFORM_DELTA, 2, src, dest, len, ndims)


def decode_doubledelta_rowmajor_8b(src, dest, len=0, ndims=0):  # noqa: A002
    return _dec_t(_lib.TRANSFORM_DOUBLEDELTA, 1, src, dest, len, ndims)


def decode_doubledelta_rowmajor_16b(src, dest, len=0, ndims=0):  # noqa: A002
    return _dec_t(_lib.TRANSFORM_DOUBLEDELTA, 2, src, dest, len, ndims)


def encode_xff_rowmajor_8b(src, len, dest, ndims, write_size=True):  # noqa: A002 (predict.h:15)
    return _enc_t(_lib.TRANSFORM_XFF, 1, src, len, dest, ndims, write_size)


def encode_xff_rowmajor_16b(src, len, dest, ndims, write_size=True):  # noqa: A002 (predict.h:24)
    return _enc_t(_lib.TRANSFORM_XFF, 2, src, len, dest, ndims, write_size)


def decode_xff_rowmajor_8b(src, dest, len=0, ndims=0):  # noqa: A002 (predict.h:17-21)
    return _dec_t(_lib.TRANSFORM_XFF, 1, src, dest, len, ndims)


def decode_xff_rowmajor_16b(src, dest, len=0, ndims=0):  # noqa: A002 (predict.h:26-30)
    return _dec_t(_lib.TRANSFORM_XFF, 2, src, dest, len, ndims)


def transform_device(kind, x, ndims, inverse=False, out=None):
    """delta ("delta") / double delta ("doubledelta") / FIRE errors ("xff", predict.h) of one
    row-major stream resident in HBM (torch uint8/uint16 tensor); inverse=True undoes it (delta
    kinds: a multi-level scan over the rows; xff: a lane per column, sequential in the rows).
    The decode's scratch is sprintz_mi355x_transform_tmp_bytes: enough for every form of the scan at any
    alignment of `x` and `out`, its contents on entry do not matter."""
    import torch
    k = {"delta": _lib.TRANSFORM_DELTA, "doubledelta": _lib.TRANSFORM_DOUBLEDELTA, "xff": _lib.TRANSFORM_XFF}[kind]
    esz = x.dtype.itemsize
    x = x.contiguous().reshape(-1)
    if out is None:
        out = torch.empty_like(x)
    stream = C.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)
    if not inverse:
        with torch.cuda.device(x.device):
            _lib.check(_lib.transform_encode_device(k, esz, x.data_ptr(), x.numel(), ndims, out.data_ptr(), stream))
    else:
        tmp = torch.empty(int(_lib.transform_tmp_bytes(k, esz, x.numel(), ndims)), dtype=torch.uint8, device=x.device)
        with torch.cuda.device(x.device):
            _lib.check(_lib.transform_decode_device(k, esz, x.data_ptr(), x.numel(), ndims, out.data_ptr(), tmp.data_ptr(), stream))
    return out


# ---- optional Huffman stage (device) ------------------------------------------------

@dataclass
class HufBatch:
    """Huffman-coded container (format: oracle/huf_oracle.c; unpinned vs the reference)."""
    data: "torch.Tensor"       # uint8 records
    offsets: "torch.Tensor"    # int64 [nchunks+1]
    tables: "torch.Tensor"     # uint8 [ceil(nchunks/64)*128]
    nchunks: int
    total_len: int
    chunk_len: int
    ndims: int

    def total_bytes(self):
        return int(self.offsets[-1].item()) + int(self.tables.numel())


def huf_compress(batch):
    """CompressedBatch -> HufBatch (entropy-codes the chunk streams on the GPU)"""
    import torch
    dev = batch.data.device
    n = batch.nchunks
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    total = batch.stream_bytes()
    huf = torch.zeros(int(_lib.huf_bound(total, n)), dtype=torch.uint8, device=dev)   # record gaps (< 4 B) read as 0
    hoffs = torch.empty(n + 1, dtype=torch.int64, device=dev)
    tables = torch.empty(((n + 63) // 64) * 128, dtype=torch.uint8, device=dev)
    tmp = torch.empty(int(_lib.huf_tmp_bytes(n)), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.huf_compress_batch(batch.data.data_ptr(), batch.offsets.data_ptr(), batch.sizes.data_ptr(), n,
                                           huf.data_ptr(), hoffs.data_ptr(), tables.data_ptr(), tmp.data_ptr(), stream))
    end = int(hoffs[-1].item())
    return HufBatch(huf[: end + _lib.READ_SLACK].clone(), hoffs, tables, n, batch.total_len, batch.chunk_len, batch.ndims)


def huf_decompress(hb, dense_capacity, align=16, rets=None):
    """HufBatch -> CompressedBatch (the exact Sprintz container again).  rets: optional int64
    tensor [nchunks] receiving each chunk's byte count, or E_CORRUPT for a damaged record."""
    import torch
    dev = hb.data.device
    n = hb.nchunks
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    cap = dense_capacity + 16 * n
    dense = torch.zeros(cap + _lib.READ_SLACK, dtype=torch.uint8, device=dev)
    offs = torch.empty(n + 1, dtype=torch.int64, device=dev)
    sizes = torch.empty(n, dtype=torch.int32, device=dev)
    tmp = torch.empty(int(_lib.compact_tmp_bytes(n)) + 64, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.huf_decompress_batch(hb.data.data_ptr(), hb.offsets.data_ptr(), hb.tables.data_ptr(), n, align,
                                             dense.data_ptr(), cap, offs.data_ptr(), sizes.data_ptr(),
                                             rets.data_ptr() if rets is not None else None, tmp.data_ptr(), stream))
    return CompressedBatch(dense, offs, sizes, n, hb.total_len, hb.chunk_len, hb.ndims)


def huf0_compress(batch):
    """CompressedBatch -> (blocks uint8 tensor, block_offsets int64 [nchunks+1]): one genuine Huff0 block per
    chunk (readable by HUF_decompress / lzbench's huff0; format of the writer: oracle/huf0_oracle.c)"""
    import torch
    dev = batch.data.device
    n = batch.nchunks
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    total = int(batch.sizes.sum().item())
    blocks = torch.zeros(int(_lib.huf0_bound(total, n)), dtype=torch.uint8, device=dev)
    boffs = torch.empty(n + 1, dtype=torch.int64, device=dev)
    tmp = torch.empty(int(_lib.huf0_tmp_bytes(n)), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.huf0_compress_batch(batch.data.data_ptr(), batch.offsets.data_ptr(), batch.sizes.data_ptr(), n,
                                            blocks.data_ptr(), boffs.data_ptr(), tmp.data_ptr(), stream))
    return blocks, boffs


def huf0_compress_exact(batch, table_log=11):
    """CompressedBatch -> (blocks uint8 tensor, block_offsets int64 [nchunks+1]) like huf0_compress, but every chunk
    has its own code table and its block is byte for byte libzstd 1.4.8's HUF_compress2(..., 255, table_log) of it
    (table_log 11 = HUF_compress; 5 .. 12).  Specification: tests/huf0_exact_model.py."""
    import torch
    dev = batch.data.device
    n = batch.nchunks
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    total = int(batch.sizes.sum().item())
    blocks = torch.zeros(int(_lib.huf0_bound(total, n)), dtype=torch.uint8, device=dev)
    boffs = torch.empty(n + 1, dtype=torch.int64, device=dev)
    tmp = torch.empty(int(_lib.huf0_exact_tmp_bytes(n)), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.huf0_compress_batch_exact(batch.data.data_ptr(), batch.offsets.data_ptr(), batch.sizes.data_ptr(), n,
                                                  int(table_log), blocks.data_ptr(), boffs.data_ptr(), tmp.data_ptr(), stream))
    return blocks, boffs


def huf0_decompress(blocks, block_offsets, out_offsets, rets=None, out=None, max_block_bytes=0):
    """Genuine Huff0 blocks (HUF_compress's output, one per chunk; torch uint8 tensor + int64 offsets
    [nchunks+1]) -> the bytes they encode, chunk c at out_offsets[c] (int64 [nchunks+1], device).
    `blocks` must be 16-byte aligned and carry 16 readable bytes past the last block.  Returns the uint8 output tensor
    (READ_SLACK bytes longer than out_offsets[-1], ready for ChunkedCodec.decompress_into).
    max_block_bytes: an upper bound of the blocks' sizes if the caller has one (a chunk's compress_bound, say) -- small
    batches size their LDS image of a block by it (sprintz_mi355x_huf0_decompress_batch_hint); 0 = unknown."""
    import torch
    dev = blocks.device
    n = block_offsets.numel() - 1
    if out is None:
        out = torch.zeros(int(out_offsets[-1].item()) + _lib.READ_SLACK, dtype=torch.uint8, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    with torch.cuda.device(dev):
        if max_block_bytes:
            tmp = torch.empty(int(_lib.huf0_decode_tmp_bytes(n)), dtype=torch.uint8, device=dev)
            _lib.check(_lib.huf0_decompress_batch_hint(blocks.data_ptr(), block_offsets.data_ptr(), n, out.data_ptr(), out_offsets.data_ptr(),
                                                       rets.data_ptr() if rets is not None else None, tmp.data_ptr(), int(max_block_bytes), stream))
        else:
            _lib.check(_lib.huf0_decompress_batch(blocks.data_ptr(), block_offsets.data_ptr(), n, out.data_ptr(), out_offsets.data_ptr(),
                                                  rets.data_ptr() if rets is not None else None, stream))
    return out


# ---- host convenience (lzbench-style, PCIe inclusive) ---------------------------

def compress_chunked(codec, data, ndims, chunk_len):
    """numpy in -> (stream bytes np.uint8, offsets np.uint64[nchunks+1])"""
    data = np.ascontiguousarray(data)
    esz = data.dtype.itemsize
    nchunks = int(_lib.num_chunks(data.size, chunk_len))
    cap = nchunks * int(_lib.compress_bound(esz, chunk_len, ndims)) + 64
    comp = np.empty(cap, np.uint8)
    offsets = np.zeros(nchunks + 1, np.uint64)
    total = _lib.compress_chunked_host(_CODEC_ID[codec], esz, _np_ptr(data), data.size, chunk_len, ndims,
                                       _np_ptr(comp), cap, _np_ptr(offsets))
    _lib.check(total)
    return comp[:total].copy(), offsets


def decompress_chunked(codec, comp, offsets, esz, ndims, chunk_len):
    comp = np.ascontiguousarray(comp, dtype=np.uint8)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    nchunks = len(offsets) - 1
    out = np.empty(nchunks * chunk_len, _NP[esz])
    n = _lib.decompress_chunked_host(_CODEC_ID[codec], esz, _np_ptr(comp), _np_ptr(offsets), nchunks, chunk_len, ndims,
                                     _np_ptr(out))
    _lib.check(n)
    return out[:n]
