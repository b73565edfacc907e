"""Filter rows against decompress + torch, on the bench's own inputs (tests/test_gpu_bench_data.py: bench_input).

For cfg2 (u16 x 8, FIRE: the headline batch), cfg3_10k (u8 x 80, delta) and cfg1 (u8 x 1, delta), with the band predicate -- columns 0
and D - 1 inside their own quartiles, mode ALL, the rest unconstrained:
  (a) sprintz_mi355x_filter_rows, mask + counts (nothing but the mask and the counts leaves the chip)
  (b) decompress_into + the equivalent torch predicate, ((x >= lo) & (x <= hi)).all(dim=1): what a caller does without (a).
      Where torch has no comparison for the element type (unsigned 16 bit), the cheapest equivalent: the same bits as int16 with
      the sign bit flipped, against bounds flipped alike -- one extra 2-byte pass, not a widening.  "torch_predicate" says which.
  (c) sprintz_mi355x_query_windows, W = 64, min + max + sum          (for information)
  (d) decompress_into alone                                          (for information)
Device events, warm-up, `--steps` timed launches per measurement; (a) and (b) alternate in one process, `--repeats` times, and
the spread of the repeats is reported.  (a) is checked against (b) once per shape.  One JSON line per shape; `--out` writes them
to a file behind a line that names the device and the commit.  Exits non-zero where (a) differs from (b), or where (a) is
not faster than (b) on cfg2, the headline batch: that is the feature's requirement.
  python tools/bench_filter.py [--steps 20] [--repeats 3] [--configs cfg2,cfg3_10k,cfg1] [--commit TEXT] [--out FILE]
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
from sprintz_amd import _lib  # noqa: E402
from rowdata import bench_input


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
    ap.add_argument("--configs", default="cfg2,cfg3_10k,cfg1")
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
        batch = cd.compress(x)
        del x
        cid = _lib.CODEC_DELTA if codec == "delta" else _lib.CODEC_XFF
        R = chunk_len // D
        MB = -(-R // 8)
        top = (1 << (8 * esz)) - 1
        out = torch.empty(nchunks * chunk_len, dtype=cd.dtype, device=dev)
        cd.decompress_into(batch.data, batch.offsets, nchunks, out)
        lo, hi = [0] * D, [top] * D
        for d in sorted({0, D - 1}):                       # the band: the column's own lower quartiles
            col = out.view(-1, D)[:, d].to(torch.int32)
            lo[d] = int(torch.kthvalue(col, int(0.25 * (col.numel() - 1)) + 1).values.item())
            hi[d] = int(torch.kthvalue(col, int(0.75 * (col.numel() - 1)) + 1).values.item())
            del col
        lo_t = torch.tensor(lo, dtype=torch.int32, device=dev).to(cd.dtype)
        hi_t = torch.tensor(hi, dtype=torch.int32, device=dev).to(cd.dtype)
        mask = torch.empty((nchunks, MB), dtype=torch.uint8, device=dev)
        counts = torch.empty(nchunks, dtype=torch.int32, device=dev)

        def run_a():
            _lib.check(_lib.filter_rows(cid, esz, batch.data.data_ptr(), batch.offsets.data_ptr(), nchunks, chunk_len, D, lo_t.data_ptr(),
                                        hi_t.data_ptr(), _lib.FILTER_ALL, 0, mask.data_ptr(), counts.data_ptr(), None, stream()))

        def predicate_native():
            v = out.view(-1, D)
            return ((v >= lo_t) & (v <= hi_t)).all(dim=1)

        if esz == 2:                                       # unsigned order = signed order of the bits with the sign bit flipped
            lo_s, hi_s = lo_t.view(torch.int16) ^ -32768, hi_t.view(torch.int16) ^ -32768

        def predicate_biased():
            v = out.view(torch.int16).view(-1, D) ^ -32768
            return ((v >= lo_s) & (v <= hi_s)).all(dim=1)
        try:
            predicate_native()
            torch.cuda.synchronize()
            predicate, form = predicate_native, "native"
        except (RuntimeError, NotImplementedError):
            predicate, form = predicate_biased, "int16 view, sign bit flipped"

        def run_b():
            cd.decompress_into(batch.data, batch.offsets, nchunks, out)
            return predicate()

        W = 64
        nwin = -(-R // W)
        mn = torch.empty((nchunks, nwin, D), dtype=cd.dtype, device=dev)
        mx = torch.empty_like(mn)
        sm = torch.empty((nchunks, nwin, D), dtype=torch.int64, device=dev)

        def run_c():
            _lib.check(_lib.query_windows(cid, esz, batch.data.data_ptr(), batch.offsets.data_ptr(), nchunks, chunk_len, D, W, 7, 0,
                                          mn.data_ptr(), mx.data_ptr(), sm.data_ptr(), None, stream()))

        def run_d():
            cd.decompress_into(batch.data, batch.offsets, nchunks, out)

        run_a()
        ref = run_b()
        torch.cuda.synchronize()
        weights = torch.tensor([1, 2, 4, 8, 16, 32, 64, 128], dtype=torch.int32, device=dev)
        ok = bool(R % 8 == 0 and torch.equal(mask.view(-1), (ref.view(-1, 8).to(torch.int32) * weights).sum(dim=1).to(torch.uint8))
                  and torch.equal(counts.to(torch.int64), ref.view(nchunks, R).sum(dim=1)))
        matching = int(ref.sum().item())
        del ref
        ta, tb = [], []
        for _ in range(args.repeats):
            ta.append(timed(run_a, args.steps))
            tb.append(timed(run_b, args.steps))
        tc, td = timed(run_c, args.steps), timed(run_d, args.steps)
        rec = {"config": name, "codec": codec, "elem_bytes": esz, "ndims": D, "chunk_len": chunk_len, "nchunks": nchunks, "ok": ok,
               "rows": nchunks * R, "rows_matching": matching, "torch_predicate": form,
               "a_filter_rows_ms": [round(t, 4) for t in ta], "b_decompress_torch_ms": [round(t, 4) for t in tb],
               "c_query_windows_w64_ms": round(tc, 4), "d_decompress_ms": round(td, 4),
               "a_min_ms": round(min(ta), 4), "b_min_ms": round(min(tb), 4),
               "a_spread_pct": round(100 * (max(ta) - min(ta)) / min(ta), 2),
               "b_spread_pct": round(100 * (max(tb) - min(tb)) / min(tb), 2),
               "b_over_a": round(min(tb) / min(ta), 3),
               "compressed_bytes": batch.total_bytes(), "decoded_bytes": nchunks * chunk_len * esz, "mask_bytes": nchunks * MB}
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del out, mask, counts, mn, mx, sm, batch, cd
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(head) + "\n")
            for rec in lines:
                f.write(json.dumps(rec) + "\n")
    if not all(r["ok"] for r in lines):
        sys.exit("filter_rows differs from decompress + torch")
    slow = [r for r in lines if r["config"] == "cfg2" and r["b_over_a"] <= 1.0]
    if slow:
        sys.exit(f"filter_rows is not faster than decompress + torch on the headline batch: b / a = {slow[0]['b_over_a']}")


if __name__ == "__main__":
    main()
