"""Compress floats against torch's quantise expression + compress_dense, on the bench's own inputs (tests/rowdata.py: bench_input).

For cfg2 (u16 x 8, FIRE: the headline batch) and cfg3_10k (u8 x 80, delta), and for each source format (float32, float16, bfloat16), the
source is the bench's integer batch x as floats, x * scale + offset in the format, and
  (a) sprintz_mi355x_compress_batch_float_dense: the source quantised inside the encoder, one call
  (b) torch's quantise expression -- nan_to_num(round((src.float() - offset) * inv_scale), nan=0).clamp(LO, HI), cast into the padded
      integer buffer -- followed by compress_dense of it: what a caller does without (a); only code the parent commit has
  (c) compress_dense of that integer buffer alone: the floor of both
Device events, warm-up, `--steps` timed launches per measurement; (a), (b) and (c) alternate in one process, `--repeats` times, and the
minimum and the spread of the repeats are reported.  (a)'s container is checked against (b)'s once per shape and format.  One JSON line
per shape and format; `--out` writes them to a file behind a line that names the device and the commit.  No threshold is fixed: the
exit status is non-zero only where (a) differs from (b).
  python tools/bench_compress_floats.py [--steps 20] [--repeats 3] [--configs cfg2,cfg3_10k] [--commit TEXT] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import sprintz_amd as sz  # noqa: E402
from sprintz_amd import _lib, rowops  # noqa: E402
from rowdata import bench_input  # noqa: E402

FORMATS = ((torch.float32, "float32"), (torch.float16, "float16"), (torch.bfloat16, "bfloat16"))
PARAMS = {2: (0.01, -300.0), 1: (0.5, -60.0)}            # (scale, offset) by element bytes: the floats stay inside every format's range


def timed(fn, steps, warmup=3):
    for _ in range(warmup):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--configs", default="cfg2,cfg3_10k")
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731
    head = {"device": torch.cuda.get_device_name(dev), "torch": torch.__version__, "commit": args.commit, "steps": args.steps, "repeats": args.repeats}
    print(json.dumps(head), flush=True)
    lines = []
    for name in args.configs.split(","):
        (codec, esz, D, chunk_len, nchunks), x = bench_input(name, dev)
        cd = sz.ChunkedCodec(codec, esz, D, chunk_len, device=dev)
        cid = _lib.CODEC_DELTA if codec == "delta" else _lib.CODEC_XFF
        n = x.numel()
        top = (1 << (8 * esz)) - 1
        scale, offset = PARAMS[esz]
        inv, off = rowops.quant_params(scale, offset, D, dev)
        xf = (x.to(torch.int32) & top).to(torch.float32).reshape(-1) * scale + offset       # (through int32: torch's uint16 lacks most arithmetic)
        del x
        ws = cd.workspace(nchunks)
        dense_a, offs_a = cd._new_container(nchunks)
        dense_b, offs_b = cd._new_container(nchunks)
        pad = torch.zeros(n * esz + _lib.READ_SLACK, dtype=torch.uint8, device=dev)
        q_view = pad[:n * esz].view(torch.uint8 if esz == 1 else torch.int16).view(-1, D)
        for dt, fname in FORMATS:
            src = xf.to(dt).contiguous()
            fmt = rowops.float_format(dt)

            def run_a():
                _lib.check(_lib.compress_batch_float_dense(cid, esz, src.data_ptr(), fmt, inv.data_ptr(), off.data_ptr(), 0, n, chunk_len, D,
                                                           ws["slots"].data_ptr(), cd.slot_stride, ws["sizes"].data_ptr(), ws["rets"].data_ptr(),
                                                           dense_a.data_ptr(), offs_a.data_ptr(), ws["tmp"].data_ptr(), stream()))

            def quantise():
                r = torch.nan_to_num(torch.round((src.view(-1, D).float() - off) * inv), nan=0.0).clamp(0, top)
                q_view.copy_(r if esz == 1 else r.to(torch.int32))                           # (uint16 through int32: the cast wraps into the same bits)

            def run_c():
                cd.compress_dense(pad, n, ws, dense_b, offs_b)

            def run_b():
                quantise()
                run_c()

            run_a()
            sizes_a = ws["sizes"].clone()
            run_b()
            torch.cuda.synchronize()
            total = int(offs_b[-1].item())
            ok = bool(torch.equal(offs_a, offs_b) and torch.equal(sizes_a, ws["sizes"]) and torch.equal(dense_a[:total], dense_b[:total]))
            ta, tb, tc = [], [], []
            for _ in range(args.repeats):
                ta.append(timed(run_a, args.steps))
                tb.append(timed(run_b, args.steps))
                tc.append(timed(run_c, args.steps))
            rec = {"config": name, "codec": codec, "elem_bytes": esz, "ndims": D, "chunk_len": chunk_len, "nchunks": nchunks, "source": fname, "ok": ok,
                   "a_compress_float_dense_ms": [round(t, 4) for t in ta], "b_torch_quantise_compress_dense_ms": [round(t, 4) for t in tb],
                   "c_compress_dense_ms": [round(t, 4) for t in tc],
                   "a_min_ms": round(min(ta), 4), "b_min_ms": round(min(tb), 4), "c_min_ms": round(min(tc), 4),
                   "a_spread_pct": round(100 * (max(ta) - min(ta)) / min(ta), 2), "b_spread_pct": round(100 * (max(tb) - min(tb)) / min(tb), 2),
                   "b_over_a": round(min(tb) / min(ta), 3), "a_over_c": round(min(ta) / min(tc), 3),
                   "source_bytes": n * src.element_size(), "integer_bytes": n * esz, "compressed_bytes": total}
            print(json.dumps(rec), flush=True)
            lines.append(rec)
            del src
        del xf, pad, q_view, dense_a, dense_b, cd, ws
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(head) + "\n")
            for rec in lines:
                f.write(json.dumps(rec) + "\n")
    if not all(r["ok"] for r in lines):
        sys.exit("compress_batch_float_dense differs from torch's quantise expression + compress_dense")


if __name__ == "__main__":
    main()
