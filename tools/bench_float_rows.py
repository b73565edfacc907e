"""Float rows against its alternatives, on the bench's headline input (tests/test_gpu_bench_data.py: bench_input("cfg2")): uint16 x 8,
FIRE, 10 KB chunks, 131 072 chunks.

For each output format (float32, float16, bfloat16), the median of `--steps` single timings after warm-up, device events around the work:
  (a) decompress_into alone: the plain decode's launch
  (b) decompress_into plus the eager torch expression (x.to(float32) * scale + offset).to(dtype): what a caller does without float_rows
  (c) the float_rows launch (sprintz_mi355x_float_rows on a preallocated output)
(c) is checked against (b) once per format, bit for bit.  Column d's scale and offset are dequantisation-like: scale 1 / 65535 * (d + 1),
offset -d.  One JSON line per format with the three times, the output bytes of each and the ratios (c) / (a) and (c) / (b); `--out` writes
them behind a line that names the device and the commit.  Exits non-zero where (c) differs from (b) or is not faster than (b).
  python tools/bench_float_rows.py [--steps 20] [--commit TEXT] [--out FILE]
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
from sprintz_amd import _lib  # noqa: E402
from rowdata import bench_input


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
    (codec, esz, D, chunk_len, nchunks), x = bench_input("cfg2", dev)
    cd = sz.ChunkedCodec(codec, esz, D, chunk_len, device=dev)
    batch = cd.compress(x)
    del x
    cid = _lib.CODEC_DELTA if codec == "delta" else _lib.CODEC_XFF
    ne = nchunks * chunk_len
    dec = torch.empty(ne, dtype=cd.dtype, device=dev)
    scale = (torch.arange(1, D + 1, dtype=torch.float32, device=dev) / 65535.0).contiguous()
    offset = (-torch.arange(D, dtype=torch.float32, device=dev)).contiguous()
    view_in = torch.int16 if esz == 2 else torch.int8
    top = (1 << (8 * esz)) - 1

    def run_a():
        cd.decompress_into(batch.data, batch.offsets, nchunks, dec)

    lines, bad = [], False
    for fmt, dt in ((_lib.FLOAT_F32, torch.float32), (_lib.FLOAT_F16, torch.float16), (_lib.FLOAT_BF16, torch.bfloat16)):
        out = torch.empty(ne, dtype=dt, device=dev)

        def run_b():
            cd.decompress_into(batch.data, batch.offsets, nchunks, dec)
            v = (dec.view(view_in).to(torch.int32) & top).to(torch.float32).view(-1, D)      # (the unsigned element: torch's uint16 lacks most operators)
            return (v * scale + offset).to(dt)

        def run_c():
            _lib.check(_lib.float_rows(cid, esz, batch.data.data_ptr(), batch.offsets.data_ptr(), nchunks, chunk_len, D, fmt, scale.data_ptr(),
                                       offset.data_ptr(), 0, out.data_ptr(), None, stream()))

        before = _lib.dispatch_counts()
        run_c()
        after = _lib.dispatch_counts()
        want = run_b()
        torch.cuda.synchronize()
        bits = torch.int32 if dt == torch.float32 else torch.int16
        ok = bool(torch.equal(out.view(bits), want.reshape(-1).view(bits))) and after["dec_fast"] - before["dec_fast"] == 1
        del want
        a, b, c = median_ms(run_a, args.steps), median_ms(run_b, args.steps), median_ms(run_c, args.steps)
        osz = out.element_size()
        rec = {"format": str(dt).replace("torch.", ""), "codec": codec, "elem_bytes": esz, "ndims": D, "chunk_len": chunk_len, "nchunks": nchunks, "ok": ok,
               "a_decompress_ms": a, "b_decompress_torch_ms": b, "c_float_rows_ms": c,
               "a_out_bytes": ne * esz, "b_out_bytes": ne * osz, "c_out_bytes": ne * osz,
               "c_over_a": round(c / a, 3), "out_bytes_c_over_a": round(osz / esz, 3), "c_over_b": round(c / b, 3),
               "c_out_gb_s": round(ne * osz / c / 1e6, 1)}
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        bad = bad or not ok or not c < b
        del out
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(head) + "\n")
            for rec in lines:
                f.write(json.dumps(rec) + "\n")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
