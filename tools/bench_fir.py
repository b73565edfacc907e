"""FIR rows against its alternatives, on the bench's headline input (tests/rowdata.py: bench_input("cfg2"): uint16 x 8, FIRE, 10 KB chunks,
131 072 chunks) and on BASELINE config 3 at 10 KB (bench_input("cfg3_10k"): uint8 x 80, delta -- a shape the generic kernel serves).

Everything in one job, every variant of a shape timed in turn, round after round (`--steps` rounds behind 3 warm-up rounds), device events around
the work; a line gives the median, the fastest and the slowest round:
  decompress                   the plain decode's launch (decompress_into) -- twice a round, first and last, as the job's own spread
  rolling_sum_W8 / _W64        rolling rows' sum: the same ring, weights of one
  diff_rows                    derive rows' diff of (up to 16) columns as int32: one weighted row back
  fir_T<T>_int32 / _float32    the filter's call on preallocated output and scratch, T = 2, 9, 33, 65, random signed taps that differ per column
  torch_T<T>_int32 / _float32  the route it replaces: the full decode, then an exact torch expression on the decoded tensor -- the sum of T
                               shifted int32 slices, each times its row of taps (addcmul_), on the edge-replicated tensor; not a float convolution
Each filter is checked against its torch route once, exactly, and its line says whether its median lies below its torch route's fastest round
(`beats_torch`).  One JSON line per measurement; `--out` writes them behind a line that names the device and the commit.  Exits non-zero where a
result differs.
  python tools/bench_fir.py [--steps 20] [--commit TEXT] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import sprintz_amd as sz  # noqa: E402
from sprintz_amd import _lib, rowops  # noqa: E402
from bench_derive import as_int32, time_rounds  # noqa: E402
from rowdata import bench_input  # noqa: E402

TAPS = (2, 9, 33, 65)


def bench_config(name, dev, steps, stream):
    (codec, esz, D, chunk_len, nchunks), x = bench_input(name, dev)
    cd = sz.ChunkedCodec(codec, esz, D, chunk_len, device=dev)
    batch = cd.compress(x)
    del x
    cid = _lib.CODEC_DELTA if codec == "delta" else _lib.CODEC_XFF
    ne = nchunks * chunk_len
    G = ne // D
    dec = torch.empty(ne, dtype=cd.dtype, device=dev)
    shape = {"config": name, "codec": codec, "elem_bytes": esz, "ndims": D, "chunk_len": chunk_len, "nchunks": nchunks}
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731

    def run_dec():
        cd.decompress_into(batch.data, batch.offsets, nchunks, dec)

    variants = [("decompress", run_dec)]
    info = {"decompress": dict(what="decompress", out_bytes=ne * esz), "decompress_again": dict(what="decompress", again=True, out_bytes=ne * esz)}
    # one output and one scratch, shared by every variant that writes ne x 4 bytes
    out = torch.empty(ne, dtype=torch.int32, device=dev)
    for W in (8, 64):
        rtmp = torch.empty(max(rowops.rolling_tmp_bytes(nchunks, W, D, esz) // 16, 1) * 2, dtype=torch.int64, device=dev)

        def run_roll(W=W, rtmp=rtmp):
            _lib.check(_lib.rolling_rows(cid, esz, batch.data.data_ptr(), batch.offsets.data_ptr(), nchunks, chunk_len, D, W, _lib.ROLL_SUM, 0, None, None,
                                         out.data_ptr(), rtmp.data_ptr(), None, stream()))
        variants.append((f"rolling_sum_W{W}", run_roll))
        info[f"rolling_sum_W{W}"] = dict(what="rolling_rows sum", window_rows=W, out_bytes=ne * 4)
    K = min(D, 16)
    wt, ut, bt = rowops.derive_forms([{c: 1} for c in range(K)], [{c: -1} for c in range(K)], 0, D, esz, dev)
    dtmp = torch.empty(max(_lib.derive_rows_tmp_bytes(esz, nchunks, D) // 8, 1), dtype=torch.int64, device=dev)

    def run_diff():
        _lib.check(_lib.derive_rows(cid, esz, batch.data.data_ptr(), batch.offsets.data_ptr(), nchunks, chunk_len, D, K, wt.data_ptr(), ut.data_ptr(), bt.data_ptr(),
                                    _lib.DERIVE_I32, None, None, None, 0, dtmp.data_ptr(), out.data_ptr(), None, stream()))
    variants.append(("diff_rows", run_diff))
    info["diff_rows"] = dict(what="derive_rows diff", ncolumns=K, out_bytes=G * K * 4)

    gen = torch.Generator().manual_seed(19)
    scale = torch.linspace(0.5, 2.0, D, device=dev)
    offset = torch.linspace(-3.0, 3.0, D, device=dev)
    pairs, bad = [], False
    for T in TAPS:
        taps = torch.randint(-400, 401, (T, D), generator=gen, dtype=torch.int32)
        tt, bt_ = rowops.fir_taps(taps, 7, D, esz, dev)
        ftmp = torch.empty(max(rowops.fir_tmp_bytes(nchunks, T, D, esz) // 16, 1) * 2, dtype=torch.int64, device=dev)
        for dtype in (torch.int32, torch.float32):
            flt = dtype != torch.int32
            label = f"T{T}_{'float32' if flt else 'int32'}"
            fmt = _lib.DERIVE_F32 if flt else _lib.DERIVE_I32

            def run_fir(T=T, tt=tt, bt_=bt_, ftmp=ftmp, fmt=fmt, flt=flt):
                _lib.check(_lib.fir_rows(cid, esz, batch.data.data_ptr(), batch.offsets.data_ptr(), nchunks, chunk_len, D, T, tt.data_ptr(), bt_.data_ptr(), fmt,
                                         ptr(scale if flt else None), ptr(offset if flt else None), None, 0, ftmp.data_ptr(), out.data_ptr(), None, stream()))

            def run_torch(T=T, tt=tt, bt_=bt_, flt=flt):
                run_dec()
                r = as_int32(dec.view(G, D))
                pad = torch.cat([r[:1].expand(T - 1, D), r])
                acc = bt_.unsqueeze(0).expand(G, D).contiguous()
                for j in range(T):
                    acc.addcmul_(pad[T - 1 - j:T - 1 - j + G], tt[j].unsqueeze(0))
                return acc.to(torch.float32) * scale + offset if flt else acc

            before = _lib.dispatch_counts()
            run_fir()
            after = _lib.dispatch_counts()
            want = run_torch()
            torch.cuda.synchronize()
            ok = bool(want.dtype == dtype and torch.equal(out.view(G, D), want.view(torch.int32)))
            del want
            bad = bad or not ok
            info[f"fir_{label}"] = dict(what="fir_rows", ntaps=T, dtype=str(dtype).split(".")[-1], family=[k for k in after if after[k] != before[k]], ok=ok,
                                        out_bytes=ne * 4)
            info[f"torch_{label}"] = dict(what="decompress + sum of shifted int32 slices", ntaps=T, dtype=str(dtype).split(".")[-1], out_bytes=ne * 4)
            variants += [(f"fir_{label}", run_fir), (f"torch_{label}", run_torch)]
            pairs.append(label)
    variants.append(("decompress_again", run_dec))
    times = time_rounds(variants, steps)
    for label in pairs:
        info[f"fir_{label}"]["beats_torch"] = bool(statistics.median(times[f"fir_{label}"]) < min(times[f"torch_{label}"]))
    lines = []
    for key, _ in variants:
        t = times[key]
        lines.append(dict(shape, variant=key, **info[key], ms=round(statistics.median(t), 4), ms_min=round(min(t), 4), ms_max=round(max(t), 4)))
        print(json.dumps(lines[-1]), flush=True)
    return lines, bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731
    head = {"device": torch.cuda.get_device_name(dev), "torch": torch.__version__, "commit": args.commit, "steps": args.steps}
    print(json.dumps(head), flush=True)
    lines, bad = [], False
    for name in ("cfg2", "cfg3_10k"):
        got, b = bench_config(name, dev, args.steps, stream)
        lines += got
        bad = bad or b
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(head) + "\n")
            for rec in lines:
                f.write(json.dumps(rec) + "\n")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
