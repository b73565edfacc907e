"""Rolling rows against its alternatives, on the bench's headline input (tests/rowdata.py: bench_input("cfg2"): uint16 x 8, FIRE, 10 KB
chunks, 131 072 chunks) and on BASELINE config 3 at 10 KB (bench_input("cfg3_10k"): uint8 x 80, delta).

The median of `--steps` single timings after 3 warm-ups, device events around the work, everything in one job:
  (a) decompress_into alone: the plain decode's launch
  (b) (a) plus the torch expression for the same result on the decoded tensor, taken as ONE sequence of rows (so the chunk seams are
      handled): unfold(0, W, 1).amin / .amax on the front-padded int32 tensor for min / max, an int64 cumsum (along the
      contiguous dimension of the transposed tensor, where torch's scan is parallel) and a shifted subtract for sum
  (c) the rolling launch with its seam pass (sprintz_mi355x_rolling_rows on preallocated outputs and scratch): min alone, max alone, sum
      alone and all three, at W = 8, 16, 64 -- and all three at the largest W the shape's history rings allow
  the float_rows float32 launch, the yardstick of a decode that writes twice the bytes, and (c) on constant data under the delta codec (all
  three ops, W = 8 and 64), where every chunk is one delta run: with the run shortcut, and -- run again with --constant-only --shortcut 0 on a
  library built with -DSPRINTZ_ROLL_RUN_SHORTCUT=0 (SPRINTZ_MI355X_LIB) -- without it
(c) is checked against (b) once per (ops, W), exactly.  One JSON line per measurement; `--out` writes them behind a line that names the
device and the commit.  Exits non-zero where (c) differs from (b) or is not faster than (b).
  python tools/bench_rolling.py [--steps 20] [--commit TEXT] [--out FILE] [--constant-only] [--shortcut 0|1]
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
from rowdata import bench_input  # noqa: E402
import rolling_model as rm  # noqa: E402

NAMES = {1: "min", 2: "max", 4: "sum", 7: "min|max|sum"}


def median_ms(fn, steps, warmup=3):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(steps):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return round(statistics.median(times), 4)


def torch_rolling(v, W, ops, top):
    """v: int32 [G, D], the decoded batch as one sequence -> {op: [G, D]}"""
    out = {}
    if ops & 3:
        for name, bit, pad in (("min", 1, top), ("max", 2, 0)):
            if ops & bit:
                win = torch.cat([v.new_full((W - 1, v.shape[1]), pad), v]).unfold(0, W, 1)
                out[name] = win.amin(-1) if name == "min" else win.amax(-1)
    if ops & 4:
        # (the scan runs along the contiguous dimension: torch scans an outer dimension of 8 columns with a thread a column)
        cs = v.t().to(torch.int64).contiguous().cumsum(1)
        cs[:, W:] -= cs[:, :-W].clone()
        out["sum"] = cs.to(torch.int32).t().contiguous()
    return out


def bench_config(name, dev, steps, stream, yardstick):
    (codec, esz, D, chunk_len, nchunks), x = bench_input(name, dev)
    cd = sz.ChunkedCodec(codec, esz, D, chunk_len, device=dev)
    batch = cd.compress(x)
    del x
    cid = _lib.CODEC_DELTA if codec == "delta" else _lib.CODEC_XFF
    ne = nchunks * chunk_len
    top = (1 << (8 * esz)) - 1
    view_in = torch.int16 if esz == 2 else torch.int8
    dec = torch.empty(ne, dtype=cd.dtype, device=dev)
    outs = {1: torch.empty(ne, dtype=cd.dtype, device=dev), 2: torch.empty(ne, dtype=cd.dtype, device=dev), 4: torch.empty(ne, dtype=torch.int32, device=dev)}
    wmax = min(rm.max_window(esz, D, False), chunk_len // D // 8 * 8)
    tmp = torch.empty(rowops.rolling_tmp_bytes(nchunks, wmax, D, esz), dtype=torch.uint8, device=dev)
    shape = {"config": name, "codec": codec, "elem_bytes": esz, "ndims": D, "chunk_len": chunk_len, "nchunks": nchunks}

    def run_a():
        cd.decompress_into(batch.data, batch.offsets, nchunks, dec)

    def decoded():
        run_a()
        return (dec.view(view_in).to(torch.int32) & top).view(-1, D)

    def launch(b, W, ops):
        _lib.check(_lib.rolling_rows(cid, esz, b.data.data_ptr(), b.offsets.data_ptr(), nchunks, chunk_len, D, W, ops, 0,
                                     outs[1].data_ptr() if ops & 1 else None, outs[2].data_ptr() if ops & 2 else None,
                                     outs[4].data_ptr() if ops & 4 else None, tmp.data_ptr(), None, stream()))

    lines, bad = [], False
    a = median_ms(run_a, steps)
    lines.append(dict(shape, what="a_decompress", ms=a, out_bytes=ne * esz))
    print(json.dumps(lines[-1]), flush=True)
    if yardstick:
        fout = torch.empty(ne, dtype=torch.float32, device=dev)
        f = median_ms(lambda: _lib.check(_lib.float_rows(cid, esz, batch.data.data_ptr(), batch.offsets.data_ptr(), nchunks, chunk_len, D, _lib.FLOAT_F32, None,
                                                         None, 0, fout.data_ptr(), None, stream())), steps)
        del fout
        lines.append(dict(shape, what="float_rows_float32", ms=f, out_bytes=ne * 4))
        print(json.dumps(lines[-1]), flush=True)
    for W in (8, 16, 64, wmax):
        for ops in ((1, 2, 4, 7) if W != wmax else (7,)):
            def run_b():
                return torch_rolling(decoded(), W, ops, top)

            def run_c():
                launch(batch, W, ops)

            before = _lib.dispatch_counts()
            run_c()
            after = _lib.dispatch_counts()
            family = [k for k in after if after[k] != before[k]]
            want = run_b()
            torch.cuda.synchronize()
            ok = all(torch.equal((outs[bit].view(view_in).to(torch.int32) & top) if bit != 4 else outs[4], want[k].reshape(-1))
                     for k, bit in (("min", 1), ("max", 2), ("sum", 4)) if ops & bit)
            del want
            b, c = median_ms(run_b, steps), median_ms(run_c, steps)
            out_bytes = ne * (esz * bin(ops & 3).count("1") + (4 if ops & 4 else 0))
            rec = dict(shape, what="rolling", ops=NAMES[ops], window_rows=W, family=family, ok=bool(ok), a_decompress_ms=a, b_decompress_torch_ms=b, c_rolling_ms=c,
                       c_out_bytes=out_bytes, c_over_a=round(c / a, 3), c_over_b=round(c / b, 4), c_out_gb_s=round(out_bytes / c / 1e6, 1),
                       lds_bytes_a_workgroup=(rm.fast_map(esz, D)[2] + rm.ring_bytes(W, D, esz)) * (rm.THREADS // rm.fast_map(esz, D)[0]) if family == ["dec_fast"]
                       else rm.ring_bytes(W, D, esz) * (rm.THREADS // rm.lanes(esz, D, False)))
            print(json.dumps(rec), flush=True)
            lines.append(rec)
            bad = bad or not ok or not c < b
    return lines, bad


def bench_constant(name, dev, steps, stream, shortcut):
    """constant data under the DELTA codec, all three ops: every chunk is one long delta run -- behind its first W + 8 rows the run shortcut
    (decode_ops.h: rolling_run_settled) skips the ring's reads and writes; a library built with -DSPRINTZ_ROLL_RUN_SHORTCUT=0 runs every block through the
    per-block step (`shortcut` says which library this is: SPRINTZ_MI355X_LIB chooses it)"""
    (_, esz, D, chunk_len, nchunks), x = bench_input(name, dev)
    del x
    cd = sz.ChunkedCodec("delta", esz, D, chunk_len, device=dev)
    ne = nchunks * chunk_len
    top = (1 << (8 * esz)) - 1
    const = cd.compress(torch.full((ne,), 0x1234 & top, dtype=torch.int32, device=dev).to(torch.int16 if esz == 2 else torch.int8).view(cd.dtype))
    outs = [torch.empty(ne, dtype=cd.dtype, device=dev), torch.empty(ne, dtype=cd.dtype, device=dev), torch.empty(ne, dtype=torch.int32, device=dev)]
    tmp = torch.empty(rowops.rolling_tmp_bytes(nchunks, 64, D, esz), dtype=torch.uint8, device=dev)
    lines = []
    for W in (8, 64):
        def run():
            _lib.check(_lib.rolling_rows(_lib.CODEC_DELTA, esz, const.data.data_ptr(), const.offsets.data_ptr(), nchunks, chunk_len, D, W, 7, 0,
                                         outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), tmp.data_ptr(), None, stream()))
        run()
        torch.cuda.synchronize()
        ok = bool(torch.all(outs[0].view(torch.int16 if esz == 2 else torch.int8).to(torch.int32) & top == 0x1234 & top)) and \
            bool(torch.equal(outs[2].view(-1, D)[:, 0].to(torch.int64), (0x1234 & top) * torch.clamp(torch.arange(ne // D, device=dev) + 1, max=W)))
        c = median_ms(run, steps)
        lines.append(dict(config=name, codec="delta", elem_bytes=esz, ndims=D, chunk_len=chunk_len, nchunks=nchunks, what="rolling_constant_data", ops=NAMES[7],
                          window_rows=W, run_shortcut=bool(shortcut), ok=ok, c_rolling_ms=c))
        print(json.dumps(lines[-1]), flush=True)
    return lines, not all(r["ok"] for r in lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--out", default=None)
    ap.add_argument("--constant-only", action="store_true", help="the constant-data timings alone")
    ap.add_argument("--shortcut", type=int, default=1, help="0: the library in use was built with -DSPRINTZ_ROLL_RUN_SHORTCUT=0 (recorded, not checked)")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731
    head = {"device": torch.cuda.get_device_name(dev), "torch": torch.__version__, "commit": args.commit, "steps": args.steps}
    print(json.dumps(head), flush=True)
    lines, bad = [], False
    for name, yardstick in (("cfg2", True), ("cfg3_10k", False)):
        if not args.constant_only:
            got, b = bench_config(name, dev, args.steps, stream, yardstick)
            lines += got
            bad = bad or b
            torch.cuda.empty_cache()
        got, b = bench_constant(name, dev, args.steps, stream, args.shortcut)
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
