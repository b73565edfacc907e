"""Gather rows against what the library offered before it -- decompress the whole batch, then index -- on the bench's inputs.

Per shape, in one process, legs alternating `--repeats` times after warm-up, HIP events around `--steps` launches:
  (a) sprintz_mi355x_gather_rows: nranges ranges of `rows` rows at uniform random starts -> [nranges, rows, D]
  (b1) decompress_into of the whole batch      (b2) out.view(-1, D)[index] with a precomputed index tensor
and read_rows of 1 % / 50 % of the batch against (b1) + a slice copy.  Reported: ms, rows delivered per second, the bytes the
algorithm reads + writes, and the decode amplification (rows decoded / rows delivered, from the starts themselves).
(a) is checked against (b) once per shape.
  python tools/bench_gather_rows.py [--steps 20] [--repeats 3] [--families default,nofast] [--out FILE]
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

import sprintz_amd as sz  # noqa: E402
from sprintz_amd import _lib  # noqa: E402
from synth import synth_torch  # noqa: E402

CONFIGS = {   # what bench.py generates for these configurations (rank 0 of 1)
    "cfg2": (("xff", 2, 8, 5120, 131072), ("walk", 2, 131072, 640, 8, 8)),
    "cfg3_10k": (("delta", 1, 80, 10240, 52429), ("walk", 1, 52429, 128, 80, 2)),
}
# (config, kind, nranges or percent, rows)
SHAPES = [("cfg2", "gather", 1024, 256), ("cfg2", "gather", 32768, 256), ("cfg2", "gather", 327680, 256),
          ("cfg3_10k", "gather", 32768, 64), ("cfg2", "read", 1, 0), ("cfg2", "read", 50, 0)]


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
    ap.add_argument("--families", default="default", help="default and / or nofast (SPRINTZ_OPT_NO_FAST: decode_kernel.h)")
    ap.add_argument("--shapes", default=None, help="indices into SHAPES, comma separated (default: all)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731
    shapes = SHAPES if args.shapes is None else [SHAPES[int(i)] for i in args.shapes.split(",")]
    lines, cache = [], {}
    for name, kind, count, rows in shapes:
        if name not in cache:
            cache.clear()
            torch.cuda.empty_cache()
            (codec, esz, D, chunk_len, nchunks), (gk, _, _, crow, _, step) = CONFIGS[name]
            x = synth_torch(gk, esz, nchunks, crow, D, dev, seed=123, step=step, chunk0=0)
            cd = sz.ChunkedCodec(codec, esz, D, chunk_len, device=dev)
            batch = cd.compress(x)
            del x
            cache[name] = (cd, batch, torch.empty(nchunks * chunk_len, dtype=cd.dtype, device=dev))
        (codec, esz, D, chunk_len, nchunks), _ = CONFIGS[name]
        cd, batch, full = cache[name]
        cid = _lib.CODEC_DELTA if codec == "delta" else _lib.CODEC_XFF
        R = chunk_len // D
        total = nchunks * R
        comp_bytes = batch.total_bytes()
        if kind == "read":
            nranges, rows = 1, total * count // 100
            starts = torch.tensor([(total - rows) // 2 + 3], dtype=torch.int64, device=dev)
        else:
            nranges = count
            g = torch.Generator(device=dev)
            g.manual_seed(nranges)
            starts = torch.randint(0, total - rows + 1, (nranges,), generator=g, device=dev, dtype=torch.int64)
        out = torch.empty((nranges, rows, D), dtype=cd.dtype, device=dev)
        index = (starts[:, None] + torch.arange(rows, device=dev)[None, :]).reshape(-1) if kind == "gather" else None
        s0 = int(starts[0].item())
        # rows decoded: every touched chunk from its row 0 to the last row the range needs from it
        # (first chunk from its row 0, whole chunks between, the last one up to the range's end: starts % R + rows in all)
        decoded = int((starts % R + rows).sum().item())
        comp_read = int(round(comp_bytes / total * decoded))       # streams are read as far as they are parsed (plus read-ahead)

        def run_a():
            _lib.check(_lib.gather_rows(cid, esz, batch.data.data_ptr(), batch.offsets.data_ptr(), nchunks, chunk_len, D,
                                        starts.data_ptr(), nranges, rows, out.data_ptr(), None, stream()))

        def run_b1():
            cd.decompress_into(batch.data, batch.offsets, nchunks, full)

        fv = full.view(torch.int8 if esz == 1 else torch.int16).view(total, D)      # torch indexes the signed view: same bits

        def run_b2():
            return fv[index] if kind == "gather" else fv[s0:s0 + rows].clone()
        for fam in args.families.split(","):
            _lib.check(_lib.set_option(_lib.OPT_NO_FAST, 1 if fam == "nofast" else 0))
            run_a()
            run_b1()
            torch.cuda.synchronize()
            if kind == "gather":                             # range by range, in slices (one comparison of the whole 1.3 GB result misreported)
                ok = True
                for i in range(0, nranges, 8192):
                    idx = starts[i:i + 8192, None] + torch.arange(rows, device=dev)[None, :]
                    ok = ok and bool(torch.equal(out[i:i + 8192].view(fv.dtype), fv[idx]))
            else:
                ok = bool(torch.equal(out[0].view(fv.dtype), fv[s0:s0 + rows]))
            ta, tb1, tb2 = [], [], []
            for _ in range(args.repeats):
                ta.append(timed(run_a, args.steps))
                tb1.append(timed(run_b1, args.steps))
                tb2.append(timed(run_b2, args.steps))
            delivered = nranges * rows
            out_bytes = delivered * D * esz
            a, b = min(ta), min(tb1) + min(tb2)
            rec = {"config": name, "kind": kind, "family": fam, "nranges": nranges, "rows": rows, "ok": ok,
                   "a_gather_ms": [round(t, 4) for t in ta], "b1_decompress_ms": [round(t, 4) for t in tb1],
                   "b2_index_ms": [round(t, 4) for t in tb2], "a_min_ms": round(a, 4), "b_min_ms": round(b, 4),
                   "b_over_a": round(b / a, 3), "a_rows_per_s": round(delivered / (a * 1e-3), 0),
                   "a_bytes": comp_read + out_bytes + nranges * 8,
                   "b_bytes": comp_bytes + 2 * nchunks * chunk_len * esz + 2 * out_bytes + (delivered * 8 if kind == "gather" else 0),
                   "amplification": round(decoded / delivered, 3),
                   "a_spread_pct": round(100 * (max(ta) - min(ta)) / min(ta), 2)}
            print(json.dumps(rec), flush=True)
            lines.append(rec)
        _lib.set_option(_lib.OPT_NO_FAST, 0)
        del out, index, starts
    if args.out:
        with open(args.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
